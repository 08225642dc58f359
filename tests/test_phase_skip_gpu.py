"""Phase-stack parity on wide-dynamic-range traces, on every engine that forms a phase stack.

The reference adds the unit phasor y / |y| of every coefficient and skips only an exact 0 / 0 (ts_pws1f_lib.c:486-494).  A trace that is
a unit spike over a background many decades below it is quiet at most coefficients while the rest of the ensemble is loud there: a
transform-based engine sees those coefficients at its rounding noise, and dropping (or mis-phasing) them moves tsPWS by ~1 / M.  The
ensembles (abi.wide_traces) put such traces -- backgrounds 1e-8 .. 1e-30, exact zeros, float subnormals, a trace scaled by 1e-30 -- among
ordinary ones, with the spikes at a different position in every trace.  Every case compares whole-call outputs (ls, tsPWS and the replica
rows where there are any) with the FP64 FIR oracle at TOL32, and asserts first that the engine it is meant for really is taken."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import jk_single_ref as ref

pytestmark = pytest.mark.gpu

TOL32 = 2e-6
HERE = os.path.dirname(os.path.abspath(__file__))

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def lib():
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    return lib


def wide(mtr, N, seed):
    return abi.wide_traces(mtr, N, seed=seed, every=max(1, mtr // 12))


def plan(kw, N):
    return tspws.Plan(tspws.resolve(abi.default_params(**kw), N), N)


def compare(lib, kw, X, times=None, srand=None):
    p = abi.default_params(**kw)
    if srand is not None:
        abi.srand(srand)
    a = abi.run_main(lib.tspws_main, p, X, times=times)
    if srand is not None:
        abi.srand(srand)
    b = abi.run_main(abi.oracle().orc_tspws_main, p, X, times=times)
    assert a["rc"] == 0 and b["rc"] == 0, (a["rc"], b["rc"])
    errs = {"ls": abi.relerr(a["ls"], b["ls"]), "tsPWS": abi.relerr(a["tsPWS"], b["tsPWS"])}
    for key in ("jk", "sub"):
        if key + "_ls" in a:
            if key == "jk":
                np.testing.assert_array_equal(a["jk_mtr"], b["jk_mtr"])
            for c in range(a[key + "_ls"].shape[0]):
                errs[f"{key}_ls[{c}]"] = abi.relerr(a[key + "_ls"][c], b[key + "_ls"][c])
                errs[f"{key}_ts[{c}]"] = abi.relerr(a[key + "_ts"][c], b[key + "_ts"][c])
    worst = max(errs, key=errs.get)
    print(f"relerr {worst} = {errs[worst]:.3e}")
    assert errs[worst] < TOL32, (worst, errs[worst])
    return a


# (id, params, traces, samples, seed): the shipped library picks the engine by size (forward.hip: spectral_size, many_trace_size)
FEW = [
    ("fir_few_48x4096", dict(), 48, 4096, 1),
    ("fir_few_40x4096_mexhat_wu15", dict(type=-3, wu=1.5), 40, 4096, 2),
]
SPECTRAL = [
    ("spectral_256x4096", dict(), 256, 4096, 3),
    ("spectral_256x4096_mexhat", dict(type=-3), 256, 4096, 4),
    ("spectral_64x16384_exact_morlet_wu15", dict(type=-2, wu=1.5), 64, 16384, 5),
    ("spectral_256x4097", dict(), 256, 4097, 6),                  # window nearly twice the trace (clipped scales: see the assertion)
    ("spectral_64x16501", dict(), 64, 16501, 7),                  # the shipped example's length: clipped scales on the dense contraction
    ("spectral_and_trace_lane_128x57344", dict(), 128, 57344, 8),  # >= 7 M samples: k_fwd_tl takes the fine octaves beside the spectrum
]


@pytest.mark.parametrize("name,kw,mtr,N,seed", FEW, ids=[c[0] for c in FEW])
def test_few_trace_fir(lib, name, kw, mtr, N, seed):
    pl = plan(kw, N)
    assert lib.tspws_hip_spectral_choice(pl.h, mtr) == pl.S
    compare(lib, kw, wide(mtr, N, seed))


@pytest.mark.parametrize("name,kw,mtr,N,seed", SPECTRAL, ids=[c[0] for c in SPECTRAL])
def test_spectral_per_trace(lib, name, kw, mtr, N, seed):
    pl = plan(kw, N)
    assert lib.tspws_hip_spectral_choice(pl.h, mtr) < pl.S
    if N == 16501:
        assert lib.tspws_hip_spectral_end_scale(pl.h) < pl.S    # scales behind the set: fwd_gemm.h
    compare(lib, kw, wide(mtr, N, seed))


# two-stage calls whose K partial-stack rows alone meet the default rule of the spectral engine (a many-trace batch of double rows).  mtr = K:
# every row is one trace, so the rows are as wide as the traces
TWO_STAGE = [
    ("rows_k70_16384_unbiased", dict(Kmax=70, unbiased=1), 70, 16384, 9),
    ("rows_k256_4096_mexhat", dict(Kmax=256, type=-3), 256, 4096, 10),
    ("rows_k256_4096_exact_morlet_unbiased_wu1", dict(Kmax=256, type=-2, unbiased=1, wu=1.0), 256, 4096, 11),
]


@pytest.mark.parametrize("name,kw,mtr,N,seed", TWO_STAGE, ids=[c[0] for c in TWO_STAGE])
def test_spectral_partial_stacks(lib, name, kw, mtr, N, seed):
    pl = plan(kw, N)
    assert lib.tspws_hip_spectral_choice(pl.h, kw["Kmax"]) < pl.S
    compare(lib, kw, wide(mtr, N, seed))


def jk_times(mtr, seed):
    rng = np.random.default_rng(seed)
    return 1262304000 + 86400 * np.sort(rng.integers(0, 3 * 365, mtr))


@pytest.mark.parametrize("kw,mtr,N", [(dict(Kmax=32, jackknife_n=4, jackknife_d=1), 32, 4096),
                                      (dict(Kmax=16, unbiased=1, jackknife_n=6, jackknife_d=2, type=-3), 48, 4096)],
                         ids=["k32_n4_d1", "k16_n6_d2_mexhat_unbiased"])
def test_spectral_rows_of_a_jackknife_call(lib, kw, mtr, N):
    """Stack + jackknife: the (C + 1) Kmax partial stacks go through k_spec_stack_rows (forward.hip: >= 64 rows, octaves of <= max(512,
    N / 16) outputs, no scale behind the set)."""
    C = abi.binomial(kw["jackknife_n"], kw["jackknife_d"])
    assert (C + 1) * kw["Kmax"] >= 64
    pl = plan(kw, N)
    assert lib.tspws_hip_spectral_first_scale(pl.h, max(512, (N + 15) // 16)) < pl.S
    assert lib.tspws_hip_spectral_end_scale(pl.h) == pl.S
    compare(lib, kw, wide(mtr, N, 12), times=jk_times(mtr, 3))


def test_single_stage_jackknife(lib):
    """jk_single.hip (per-class stacks on the few-trace kernels) against the trace-order restatement from oracle primitives."""
    mtr, N, n, d = 60, 4096, 4, 1
    X = wide(mtr, N, 13)
    times = ref.leap_times(mtr, seed=5)
    kw = dict(type=-2)
    got = abi.run_main(lib.tspws_main, abi.default_params(jackknife_n=n, jackknife_d=d, **kw), X, times=times)
    assert got["rc"] == 0
    p, Xp, _ = ref.prologue(abi.default_params(**kw), X)
    sel = ref.selection(times[:Xp.shape[0]], n, d)
    wl, wt, wm = ref.Restatement(p, Xp).replicas(sel)
    np.testing.assert_array_equal(got["jk_mtr"], wm)
    errs = [max(abi.relerr(got["jk_ts"][c], wt[c]), abi.relerr(got["jk_ls"][c], wl[c])) for c in range(len(wm)) if wm[c]]
    print(f"replica relerr {max(errs):.3e}")
    assert max(errs) < TOL32
    compare(lib, kw, X)


@pytest.mark.parametrize("kw,mtr", [(dict(subsmpl_N=3, subsmpl_p=0.7), 256), (dict(subsmpl_N=2, subsmpl_p=0.5, Kmax=8, unbiased=1), 96)],
                         ids=["single_stage_256", "two_stage_k8"])
def test_masked_subsampling(lib, kw, mtr):
    compare(lib, kw, wide(mtr, 4096, 14), srand=7)


def test_reference_fixture(lib):
    """tspws_main against the reference's own outputs on the seeded wide ensemble of tests/golden/ref_wide256.npz (256 x 4096: the
    spectral engine by size)."""
    from test_wide_range_cpu import WIDE_CASES, wide_fixture
    g, X = wide_fixture()
    pl = plan({}, X.shape[1])
    assert lib.tspws_hip_spectral_choice(pl.h, X.shape[0]) < pl.S
    for name, kw in WIDE_CASES:
        r = abi.run_main(lib.tspws_main, abi.default_params(**kw), X)
        e = max(abi.relerr(r["ls"], g[f"{name}/ls"]), abi.relerr(r["tsPWS"], g[f"{name}/tsPWS"]))
        print(f"{name}: relerr {e:.3e}")
        assert r["rc"] == 0 and e < TOL32, (name, e)


def test_repeatable_bit_for_bit(lib):
    """The same adversarial ensemble twice gives bit-identical float outputs (no atomics in the order of the phase sums)."""
    for kw, mtr, N in ((dict(), 256, 4096), (dict(Kmax=256, unbiased=1), 256, 4096)):
        X = wide(mtr, N, 15)
        a = abi.run_main(lib.tspws_main, abi.default_params(**kw), X)
        b = abi.run_main(lib.tspws_main, abi.default_params(**kw), X)
        np.testing.assert_array_equal(a["ls"], b["ls"])
        np.testing.assert_array_equal(a["tsPWS"], b["tsPWS"])


@pytest.mark.parametrize("engine", ["fir", "spectral"])
def test_engine_pinned(engine):
    """TSPWS_ENGINE=fir (every scale of a many-trace batch on k_fwd_tl / the few-trace kernels) and =spectral (even small batches and
    partial stacks through the spectrum) in a child process each: tests/phase_skip_engine.py."""
    env = dict(os.environ, TSPWS_ENGINE=engine)
    r = subprocess.run([sys.executable, os.path.join(HERE, "phase_skip_engine.py"), engine], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("PHASE_SKIP_DONE")]
    assert r.returncode == 0 and lines, r.stdout[-3000:] + r.stderr[-3000:]
    assert float(lines[0].split()[1]) < TOL32
