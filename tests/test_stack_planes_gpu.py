"""GPU parity of the two FP64 planes behind every output -- linear stack ST = sum_t Y_t, phase stack PS = sum_t Y_t / |Y_t| -- on the engines
that never hand out per-trace coefficients: k_fwd_tl (fused stacks per 64-trace block), the spectral chain (stacks fused into the inverse
passes, k_spec_fixup), k_fwd_gemm + k_gemm_reduce (the clipped scales), k_fwd_poly<., 2> in the tl layout, k_accumulate_parts in all its
modes and the fused few-trace form of k_fwd_lds.  Plan.stacks (tspws_hip_stacks_float / _double) against tests/stack_planes_ref.py: a
longdouble CPU reference of the same sums from the oracle's coefficients, with a bound at EVERY coefficient that is the suite's own 1e-11 on
the per-trace coefficients carried through the sums (no new number; see stack_planes_ref.py, and test_stack_planes_cpu.py for what the
bound rejects and admits).  The float32 outputs the rest of the suite judges let a float phase normalisation, float coefficients or one
missing phasor through; these do not.

Cases, routes and the child process are in tests/stack_planes_engine.py.  Measured ratios: profiles/stack_planes_parity.txt."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import stack_planes_engine as eng
from conftest import SWEEPS_LIB

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def tp():
    assert tspws.load().tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    import torch
    assert torch.cuda.is_available()
    if os.environ.get("TSPWS_ENGINE") or os.environ.get("TSPWS_PART_MB"):
        pytest.fail("TSPWS_ENGINE / TSPWS_PART_MB are set in the environment: the in-process cases test the default rule")
    return tspws


def ids(cases):
    return [eng.name_of(c) for c in cases]


# ---- shipped library, in process -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", eng.DEFAULT, ids=ids(eng.DEFAULT))
def test_default_rule_many_trace_planes(tp, c):
    """The default rule on ensembles above its thresholds: spectral chain for the D >= 32 octaves (two-voice frames: D >= 16), k_fwd_tl for the
    finer ones, the contraction for the clipped scales; partial last blocks, float and double input, holes, V = 7."""
    eng.run_case(tp, c)


@pytest.mark.parametrize("c", eng.FEW_FUSED, ids=ids(eng.FEW_FUSED))
def test_few_trace_fused_planes(tp, c):
    """k_fwd_lds with the stacks fused per slice of fuse_tps traces, k_fwd_poly beside it, k_accumulate_parts adding the slice planes."""
    eng.run_case(tp, c)


@pytest.mark.parametrize("c", eng.DOUBLE_DEFAULT, ids=ids(eng.DOUBLE_DEFAULT))
def test_double_rows_planes(tp, c):
    """tspws_hip_stacks_double on the FP64 partial stacks of a two-stage call: 300 rows (many-trace path by the default rule) and the
    headline's ten rows (one fused slice written straight into ST / PS)."""
    eng.run_case(tp, c)


@pytest.mark.parametrize("c", eng.EXACT_DEFAULT, ids=ids(eng.EXACT_DEFAULT))
def test_exact_properties_of_the_planes(tp, c):
    eng.run_case(tp, c)


def test_binding_refuses_what_the_entry_points_cannot_see(tp):
    import torch
    N = 2048
    pl = tp.Plan(tp.resolve(eng.abi.default_params(), N), N)
    for bad in (torch.zeros((3, N), dtype=torch.float16, device="cuda"), torch.zeros((3, N + 1), dtype=torch.float32, device="cuda"),
                torch.zeros((0, N), dtype=torch.float32, device="cuda"), torch.zeros((3, N), dtype=torch.float64)):
        with pytest.raises(tp.TspwsError):
            pl.stacks(bad)


# ---- pinned engines and budgets: one fresh child process per pin ---------------------------------------------------------------------------
def child(group):
    env, sweeps, timeout, cases = eng.GROUPS[group]
    e = dict(os.environ)
    e.update(env)
    if sweeps:
        assert os.path.exists(SWEEPS_LIB), "build it: make -C ts-pws_amd sweeps"
        e["TSPWS_LIB_PATH"] = SWEEPS_LIB
    # (a child that runs into its time limit or dies on a signal ends the session: nothing more is started on a device that may be at fault)
    try:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "stack_planes_engine.py"), group], capture_output=True,
                           text=True, timeout=timeout, env=e)
    except subprocess.TimeoutExpired as err:
        pytest.exit(f"stack_planes_engine.py {group} ran into its time limit ({err}): nothing more is started on the device", returncode=3)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    if r.returncode < 0:
        pytest.exit(f"stack_planes_engine.py {group} died on signal {-r.returncode}: nothing more is started on the device\n{tail}", returncode=3)
    assert r.returncode == 0, (group, r.returncode, tail)
    done = [l.split() for l in r.stdout.splitlines() if l.startswith("STACK_PLANES_DONE")]
    assert done and done[0][1] == group, tail
    assert int(done[0][3]) == 0 and int(done[0][2]) == len(cases), tail


def test_spectral_engine_pinned():
    """TSPWS_ENGINE=spectral on ensembles below the default thresholds (66 x 16501, 100 x 3000 with holes, 130 x 1501, 64 x 1024, V = 7) and on 80 /
    200 FP64 partial rows."""
    child("spectral")


def test_fir_engine_pinned():
    """TSPWS_ENGINE=fir: the pure trace-lane path by the shipped size rule -- decompositions tl[1] (4 and 7 blocks) and tl[0] (13 blocks, the
    last with 32 traces); at N = 16501 the clipped scales run on k_fwd_poly<., 2> in the tl layout."""
    child("fir")


@pytest.mark.parametrize("group", ["partmb_fir", "partmb"])
def test_small_partials_budget(group):
    """TSPWS_PART_MB=16: several batches with a shorter last one on the few-trace kernels (planes added under `keep`) and in the trace-lane pass."""
    child(group)


def test_contraction_order():
    """TSPWS_GEMM_ORDER=0, 1, 2 (sweeps build) on 300 x 4097: the contraction in front of, behind and beside the trace-lane kernel."""
    for o in (0, 1, 2):
        child(f"gemm{o}")


def test_every_octave_spectral():
    """TSPWS_SPEC_NSMAX=2^30 (sweeps build): every octave with D >= 8 through the spectrum."""
    child("nsmax")


# ---- sweeps build, switches that are read at every call (in process) -----------------------------------------------------------------------
def _single_stage_list():
    import test_hip_parity
    marks = [m for m in test_hip_parity.test_many_trace_single_stage_vs_oracle.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "kw,N,mtr"
    return list(marks[0].args[1])


SINGLE_STAGE = _single_stage_list()
FORCED = dict(path="forced")


def forced_case(kw, N, mtr, seed=41, tag=""):
    kw = dict(kw)
    K = kw.pop("Kmax", 0)          # two-stage with many groups: the K FP64 partial stacks are the many-trace batch
    kw.pop("unbiased", None)       # (the weighting is not part of the planes)
    kw.pop("wu", None)
    return eng.case(kw, mtr, N, seed, FORCED, rows=K or None, tag=tag)


@pytest.mark.parametrize("kw,N,mtr", SINGLE_STAGE, ids=[f"{m}x{n}-{i}" for i, (k, n, m) in enumerate(SINGLE_STAGE)])
def test_forced_trace_lane_planes(sweeps, tp, monkeypatch, kw, N, mtr):
    """The parameter list of test_hip_parity.py::test_many_trace_single_stage_vs_oracle under TSPWS_TL_MIN=64: the same shapes, FP64 per scale
    instead of float per call."""
    assert len(SINGLE_STAGE) == 12
    monkeypatch.setenv("TSPWS_TL_MIN", "64")
    eng.run_case(sweeps[0], forced_case(kw, N, mtr, tag="TSPWS_TL_MIN=64"), "sweeps")


@pytest.mark.parametrize("batch", ["64", "128"])
@pytest.mark.parametrize("N,mtr", [(4097, 300), (2048, 200)])
def test_batches_add_to_the_planes_of_the_first(sweeps, tp, monkeypatch, N, mtr, batch):
    """TSPWS_TL_BATCH=64 / 128: later batches add to the planes of the first (`keep`), the last one is partial; at N = 4097 (default rule:
    spectral) the run buffer of the contraction is reused batch after batch."""
    monkeypatch.setenv("TSPWS_TL_MIN", "64")
    monkeypatch.setenv("TSPWS_TL_BATCH", batch)
    eng.run_case(sweeps[0], forced_case(dict(), N, mtr, seed=47, tag=f"TSPWS_TL_BATCH={batch}"), "sweeps")


@pytest.mark.parametrize("pick", ["0", "1"])
@pytest.mark.parametrize("kw,N,mtr", [(dict(), 2048, 200), (dict(w0=eng.TWO_PI), 4096, 129)])
def test_both_decompositions(sweeps, tp, monkeypatch, kw, N, mtr, pick):
    """TSPWS_TL_PICK=0 / 1: both decompositions of the trace-lane path (octaves of >= 33 / >= 129 outputs on k_fwd_tl) on batches the size rule
    leaves to the FIR kernels."""
    monkeypatch.setenv("TSPWS_TL_MIN", "64")
    monkeypatch.setenv("TSPWS_TL_PICK", pick)
    c = forced_case(kw, N, mtr, seed=48, tag=f"TSPWS_TL_PICK={pick}")
    c["expect"] = dict(path="tl", pick=int(pick))
    eng.run_case(sweeps[0], c, "sweeps")


@pytest.mark.parametrize("K,N", eng.DOUBLE_SMALL)
def test_double_rows_forced_onto_the_trace_lane_path(sweeps, tp, monkeypatch, K, N):
    """80 / 200 FP64 partial rows: by the default rule batches this small stay on the few-trace kernels; TSPWS_TL_MIN=64 sends them down the
    many-trace path (the spectral pin does the same in the child of test_spectral_engine_pinned)."""
    monkeypatch.setenv("TSPWS_TL_MIN", "64")
    eng.run_case(sweeps[0], eng.case(dict(), 0, N, 76, FORCED, rows=K, tag="TSPWS_TL_MIN=64"), "sweeps")
