"""Helper of tests/test_filter_traces_gpu.py and its child process: the ensembles of the coherence filter's tests and the checker's rows for
them.  The parity batch is B = 5 ensembles of 0, 1, 2, 3 and 70 traces (the 70 cross a 64-trace block and eight slab borders), trace 16
all zero (its phasor is skipped and its row is zero).  The budget batch adds a sixth ensemble of 150 traces at N = 2048: its 150 sets of
8160 complex coefficients, 19.6 MB, exceed TSPWS_PART_MB=16 (the smallest budget; the library reads it once per process) alone, so it takes
the transform-twice path, and the six ensembles take two rounds where the default budget takes one.  As a program, argv[1] = an .npz path:
runs Plan.filter_traces on the budget batch (loo = 0, then loo = 1) under the environment's budget and writes the outputs and the stats there
for the parent to compare.  Prints FILTER_DONE <rounds> <twice>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import filter_traces_ref as ftr

tspws = importlib.import_module("ts-pws_amd")

COUNTS = (0, 1, 2, 3, 70)
FIRST = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
T = int(FIRST[-1])
ZERO = 16                      # the all-zero trace, inside the 70-trace ensemble
BIG = 150
FRAMES = {"morlet2048": (dict(), 2048), "morlet1501": (dict(), 1501), "mexhat2048": (dict(type=-3), 2048)}
PARITY = ftr.PARITY


def traces(N, big=False, seed=5):
    X = abi.synth_traces(T + (BIG if big else 0), N, seed=seed)
    X[ZERO] = 0
    return X


def first_of(big=False):
    return np.concatenate([FIRST, [T + BIG]]).astype(np.int64) if big else FIRST


def make_plan(name, **kw):
    frame_kw, N = FRAMES[name]
    return tspws.Plan(tspws.resolve(abi.default_params(**frame_kw, **kw), N), N)


def stage_of(M, Kmax):
    """(two-stage?, K) of an ensemble of M traces by the library's rule (tspws_is_two_stage)."""
    two = bool(Kmax) and Kmax <= M
    return two, (Kmax if two else M)


def want_rows(fr, hY, first, wu, unbiased, Kmax=0, loo=False):
    """The checker's filtered traces [T][N] (float64; NaN where the call leaves a row out) from the sets hY[T][ncoef] of the traces."""
    first = np.asarray(first)
    want = np.full((int(first[-1] - first[0]), fr.N), np.nan)
    for b in range(len(first) - 1):
        a, e = int(first[b] - first[0]), int(first[b + 1] - first[0])
        M = e - a
        if not M or (loo and M < 2):
            continue
        two, K = stage_of(M, Kmax)
        PS = ftr.phase_stack(ftr.group_sums(hY[a:e], Kmax) if two else hY[a:e])
        want[a:e] = ftr.filtered_rows(fr, hY[a:e], PS, K, wu, unbiased, loo).astype(np.float64)
    return want


def check_rows(got, want, what=""):
    """NaN rows exactly where defined; per row max |diff| / max |row| <= PARITY (a zero row: exactly zero).  Returns the worst ratio."""
    assert got.shape == want.shape, (got.shape, want.shape)
    worst = 0.0
    for i in range(len(want)):
        if np.isnan(want[i]).all():
            assert np.isnan(got[i]).all(), (what, i, "a row that is left out must be NaN")
            continue
        assert np.isfinite(got[i]).all(), (what, i)
        top = np.abs(want[i]).max()
        diff = np.abs(got[i].astype(np.float64) - want[i]).max()
        if top == 0:
            assert diff == 0, (what, i, "the zero trace's row must be zero")
            continue
        worst = max(worst, diff / top)
        assert diff <= PARITY * top, (what, i, diff / top)
    return worst


def run_budget(torch):
    """(out loo=0, stats, out loo=1, stats) of the budget batch at N = 2048 on NaN-filled outputs."""
    pl = make_plan("morlet2048")
    X = torch.from_numpy(traces(2048, big=True)).cuda()
    f = first_of(big=True)
    o0 = pl.filter_traces(X, f).cpu().numpy()
    s0 = pl.filter_traces_stats()
    o1 = pl.filter_traces(X, f, loo=True).cpu().numpy()
    s1 = pl.filter_traces_stats()
    return o0, s0, o1, s1


if __name__ == "__main__":
    import torch

    o0, s0, o1, s1 = run_budget(torch)
    np.savez(sys.argv[1], o0=o0, o1=o1, rounds=[s0["rounds"], s1["rounds"]], twice=[s0["twice"], s1["twice"]], rows=[s0["rows"], s1["rows"]])
    print("FILTER_DONE", s0["rounds"], s0["twice"], flush=True)
