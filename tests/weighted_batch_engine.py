"""Helpers of tests/test_weighted_stack_batch_gpu.py and its child process: the real-weighted stacks (Plan.weighted_stack_batch) on the batch of
tests/boot_batch_engine.py -- ensembles of 1, 3, 5, 8, 0 and 67 traces (one trace, both sides of the 4-trace and 8-trace loops, an empty
ensemble, enough traces for the many-trace forward engine) from h_first[0] = 2 in an array with ld = N + 5, the same traces, frames and weight
modes -- and ONE weight matrix of 17 rows whose first M rows are the case M (a row does not depend on the other rows, so the expected rows of
tests/weighted_batch_ref.py are computed once per frame and weight mode and shared):
  row 0, rows 7 .. 16   uniform random in [0.01, 3), one weight in five an exact zero
  row 1                 all zero (n+ = 0: zero rows, count 0, Keff 0)
  row 2                 a single positive weight, 0.7 (the K = 1 rule)
  row 3                 all ones
  row 4                 all 0.25
  row 5                 a 0/1 row
  row 6                 1e-6 .. 1e6: per ensemble a geometric progression over its traces (one trace: 1e-6)
Outputs hold NaN (counts: 99) before every call: an unwritten row fails.
As a program, argv[1] = "budget", argv[2] = an .npz path: the Morlet N = 2048 batch with M = 17 under the TSPWS_PART_MB of the environment (the
library reads it once per process); with the smallest budget the call must take several rounds (85 plane pairs of 8160 coefficients are
22 MB), and the rows are written to argv[2] for the parent to compare.  Prints WEIGHTED_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import boot_batch_engine as bbe
import weighted_batch_ref as wbr

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")

SIZES, FIRST, PAD, MMAX, FRAMES, WEIGHTS = bbe.SIZES, bbe.FIRST, bbe.PAD, bbe.MMAX, bbe.FRAMES, bbe.WEIGHTS
ROW_ZERO, ROW_ONE, ROW_ONES, ROW_QUARTER, ROW_MASK, ROW_WIDE = 1, 2, 3, 4, 5, 6
NONEMPTY = [b for b, mb in enumerate(SIZES) if mb]

_weights, _stacks, _expected, _plans = [], {}, {}, {}
traces, params = bbe.traces, bbe.params


def weights():
    """The weight matrix [17][84] (float64) of the module's batch."""
    if not _weights:
        rng = np.random.default_rng(52)
        T = sum(SIZES)
        w = rng.uniform(0.01, 3.0, (MMAX, T))
        w[rng.random((MMAX, T)) < 0.2] = 0.0
        w[ROW_MASK] = rng.random(T) < 0.5
        c0 = 0
        for mb in SIZES:
            if mb:
                w[ROW_ZERO, c0:c0 + mb] = 0
                w[ROW_ONE, c0:c0 + mb] = 0
                w[ROW_ONE, c0 + min(2, mb - 1)] = 0.7
                w[ROW_ONES, c0:c0 + mb] = 1
                w[ROW_QUARTER, c0:c0 + mb] = 0.25
                w[ROW_WIDE, c0:c0 + mb] = 10.0 ** (-6 + 12 * np.arange(mb) / max(1, mb - 1))
            c0 += mb
        w[0, 0] = 1.5  # (the one-trace ensemble takes part in the case M = 1)
        _weights.append(np.ascontiguousarray(w))
    return _weights[0]


def expected(frame, weight):
    """Expected ls[B][17][N], ts[B][17][N], n+[B][17], Keff[B][17] of the module's batch (computed once; do not modify)."""
    if (frame, weight) not in _expected:
        _expected[frame, weight] = wbr.expected(params(frame, weight), traces(frame), FIRST, weights(), _stacks.setdefault(frame, {}))
    return _expected[frame, weight]


def plan_of(torch, frame, weight):
    """(Plan, padded device array) of a frame and weight mode."""
    N = FRAMES[frame][1]
    if (frame, weight) not in _plans:
        X = traces(frame)
        buf = torch.zeros((X.shape[0], N + PAD), dtype=torch.float32, device="cuda")
        buf[:, :N] = torch.from_numpy(X).cuda()
        _plans[frame, weight] = (tspws.Plan(params(frame, weight), N), buf)
    return _plans[frame, weight]


def run(torch, frame, weight, w, buf=None):
    """One batched call on the padded device array (or on `buf`, an array of the same shape); outputs held NaN (counts: 99) before it."""
    pl, own = plan_of(torch, frame, weight)
    r = dict(pl=pl, buf=own if buf is None else buf, N=FRAMES[frame][1], w=np.ascontiguousarray(w, dtype=np.float64), frame=frame, weight=weight)
    return call(torch, r)


def call(torch, r):
    """The batched call of `r` (again) on NaN-filled outputs."""
    B, M, N = len(SIZES), r["w"].shape[0], r["N"]
    nan = float("nan")
    sl = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    st = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    sm = np.full((B, M), 99, np.uint32)
    out = r["pl"].weighted_stack_batch(r["buf"][:, :N], FIRST, r["w"], sl, st, sm)
    torch.cuda.synchronize()
    assert out[0] is sl and out[1] is st and out[2] is sm and len(out) == 4
    r.update(sl=sl.cpu().numpy(), st=st.cpu().numpy(), sm=sm, keff=out[3], stats=r["pl"].weighted_stack_batch_stats())
    return r


def check_counts(r):
    """What every case shares: every row written, the counts are the positive weights, Keff is 0 exactly where the count is, empty ensembles
    and rows without weight are exactly zero."""
    for k in ("sl", "st", "keff"):
        assert np.isfinite(r[k]).all(), f"{k}: rows the call did not write (NaN)"
    c0 = 0
    for b, mb in enumerate(SIZES):
        K = (r["w"][:, c0:c0 + mb] > 0).sum(axis=1)
        np.testing.assert_array_equal(r["sm"][b], K)
        np.testing.assert_array_equal(r["keff"][b] == 0, K == 0)
        assert (r["keff"][b] <= K * (1 + 1e-15)).all() and (r["keff"][b][K > 0] >= 1 - 1e-15).all()
        for m in np.flatnonzero(K == 0):
            assert not (r["sl"][b, m] != 0).any() and not (r["st"][b, m] != 0).any(), (b, m)
        c0 += mb


def check(r, want=None):
    """Worst relerr of the rows of `r` against tests/weighted_batch_ref.py (`want`: its expected() for other weights than the first M rows of
    weights()); prints every ensemble's figure.  The counts must be exact, Keff within 1e-15 relative."""
    M = r["w"].shape[0]
    if want is None:
        assert np.array_equal(r["w"], weights()[:M])
        want = expected(r["frame"], r["weight"])
    check_counts(r)
    wl, wt, wk, we = want
    np.testing.assert_array_equal(r["sm"], wk[:, :M])
    assert (np.abs(r["keff"] - we[:, :M]) <= 1e-15 * we[:, :M]).all(), (r["keff"], we[:, :M])
    worst = 0.0
    for b, mb in enumerate(SIZES):
        eb = 0.0
        for m in range(M):
            if not wk[b, m]:
                continue
            assert np.abs(wl[b, m]).max() > 0 and np.abs(wt[b, m]).max() > 0, (b, m)  # (the comparison is not between two zero rows)
            el, et = abi.relerr(r["sl"][b, m], wl[b, m]), abi.relerr(r["st"][b, m], wt[b, m])
            assert np.isfinite(el) and np.isfinite(et), (b, m)
            print(f"    ensemble {b} row {m}: relerr ls {el:.3e} ts {et:.3e} Keff {we[b, m]:.6g}")
            eb = max(eb, el, et)
        print(f"  ensemble {b} ({mb} traces): worst relerr {eb:.3e}")
        worst = max(worst, eb)
    return worst


if __name__ == "__main__":
    import torch

    if sys.argv[1] != "budget":
        raise SystemExit(f"unknown mode {sys.argv[1]}")
    r = run(torch, "morlet2048", "biased", weights())
    check_counts(r)
    st = r["stats"]
    assert st["shared"] == 5 and st["empty"] == 1 and st["rows"] == 5 * MMAX, st
    np.savez(sys.argv[2], sl=r["sl"], st=r["st"], sm=r["sm"], keff=r["keff"], rounds=st["rounds"])
    print("WEIGHTED_DONE", st["rounds"], flush=True)
