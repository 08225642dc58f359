"""GPU parity of the inverse frame transform, scale by scale, at FP64, on every launch form of tspws_hip_inverse: the four bodies of k_inv_poly
(LDS-staged, the three-frame GEN form, wave-uniform, per-lane with its scalar tail), both work lists (one item per scale / per octave), the
combining kernel, NREC = 1 and 2, grid.y offsets, the odd last set and the loop over chunks of 32768 pairs.  Plan.inverse against
tests/inverse_rows_ref.py: a longdouble CPU reference per scale from the device's own dual taps, with a bound at EVERY sample that follows
from the number of multiply-adds alone (no number of its own; see inverse_rows_ref.py, and test_inverse_rows_cpu.py for what the bound
rejects and admits).  The one global relerr < 1e-11 on the sum over scales that the suite had before lets a scale that is wrong at the 1e-9
level through, the float32 outputs one that is wrong at 1e-4; these do not.

Cases, routes and the child process are in tests/inverse_rows_engine.py.  Measured ratios: profiles/inverse_rows_parity.txt."""
import importlib
import os
import subprocess
import sys

import pytest

import inverse_rows_engine as eng
from conftest import SWEEPS_LIB

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def tp():
    assert tspws.load().tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    import torch
    assert torch.cuda.is_available()
    return tspws


@pytest.mark.parametrize("c", eng.CASES, ids=[eng.name_of(c) for c in eng.CASES])
def test_rows_of_every_launch_form(tp, c):
    """Shipped library: full, single-scale and impulse sets in one call, the first 1 / 2 / 3 / 4 / 7 sets in calls of their own, every set
    alone; the route asserted first; twice / zero set / x2 exact."""
    eng.run_case(tp, c)


def test_more_than_32768_pairs(tp):
    """65539 sets at N = 64: the second pass of the chunk loop (one pair) and the odd tail behind it."""
    eng.run_big(tp)


def test_binding_refuses_what_the_entry_point_cannot_see(tp):
    import numpy as np
    import torch
    N = 2048
    pl = tp.Plan(tp.resolve(eng.abi.default_params(), N), N)
    info = pl.inverse_info()
    assert set(info) == {"items", "per_scale", "waves", "waves_lds", "waves_fast", "generic"} and info["generic"] == 0 and info["items"] == pl.S
    for bad in (np.zeros((2, pl.ncoef)), np.zeros((2, pl.ncoef + 1), np.complex128), np.zeros(pl.ncoef, np.complex128), np.zeros((0, pl.ncoef), np.complex128),
                torch.zeros((2, pl.ncoef), dtype=torch.complex128), torch.zeros((2, pl.ncoef), dtype=torch.complex64, device="cuda"),
                torch.zeros((2, 2 * pl.ncoef), dtype=torch.complex128, device="cuda")[:, ::2], [[0j] * pl.ncoef]):
        with pytest.raises(tp.TspwsError):
            pl.inverse(bad)
    x = pl.inverse(torch.zeros((3, pl.ncoef), dtype=torch.complex128, device="cuda"))
    assert isinstance(x, torch.Tensor) and x.dtype == torch.float64 and tuple(x.shape) == (3, N) and not x.any()


# ---- sweeps build: one fresh child process per switch --------------------------------------------------------------------------------------
_children = {}


def child(group):
    """The digests {case: sha256} a child printed; runs it once per session."""
    if group in _children:
        return _children[group]
    env = eng.GROUPS[group][0]
    e = {k: v for k, v in os.environ.items() if k not in eng.SWITCHES}
    e.update(env)
    assert os.path.exists(SWEEPS_LIB), "build it: make -C ts-pws_amd sweeps"
    e["TSPWS_LIB_PATH"] = SWEEPS_LIB
    # (a child that runs into its time limit or dies on a signal ends the session: nothing more is started on a device that may be at fault)
    try:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "inverse_rows_engine.py"), group], capture_output=True,
                           text=True, timeout=eng.CHILD_TIMEOUT, env=e)
    except subprocess.TimeoutExpired as err:
        pytest.exit(f"inverse_rows_engine.py {group} ran into its time limit ({err}): nothing more is started on the device", returncode=3)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    if r.returncode < 0:
        pytest.exit(f"inverse_rows_engine.py {group} died on signal {-r.returncode}: nothing more is started on the device\n{tail}", returncode=3)
    assert r.returncode == 0, (group, r.returncode, tail)
    done = [l.split() for l in r.stdout.splitlines() if l.startswith("INVERSE_ROWS_DONE")]
    assert done and done[0][1] == group, tail
    assert int(done[0][3]) == 0 and int(done[0][2]) == len(eng.SWEEP_CASES), tail
    dig = {l.split()[2]: l.split()[3] for l in r.stdout.splitlines() if l.startswith("INVERSE_ROWS_DIGEST")}
    assert len(dig) == len(eng.SWEEP_CASES), tail
    _children[group] = dig
    return dig


@pytest.mark.parametrize("group", list(eng.GROUPS))
def test_sweeps_switches_hold_the_same_bound(group):
    """N = 4096 default, N = 2048 Mexican hat and N = 4097 under no switch, TSPWS_INV_SPLIT=0 / 1, TSPWS_INV_LDS=0, TSPWS_INV_LDS_MAXD=32 (the
    LDS-staged form with 2 .. 32 lanes per phase, which the shipped rule never picks) and TSPWS_INV_GENERIC=1."""
    child(group)


def test_lds_staged_form_is_bit_identical_to_the_per_lane_form():
    """csrc/inv_poly.h: "Same additions in the same order as the per-lane form: bit-identical outputs" -- every row of every call of the three
    cases, TSPWS_INV_LDS=0 against no switch (D = 1 staged) and TSPWS_INV_LDS_MAXD=32 (every D <= 32 staged) against TSPWS_INV_LDS=0."""
    default, lds0, maxd32 = child("default"), child("lds0"), child("maxd32")
    assert lds0 == default, ("TSPWS_INV_LDS=0 against the default", lds0, default)
    assert maxd32 == lds0, ("TSPWS_INV_LDS_MAXD=32 against TSPWS_INV_LDS=0", maxd32, lds0)
