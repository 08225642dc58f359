"""Helpers of tests/test_bootstrap_batch_gpu.py and its child process: the batched bootstrap (Plan.bootstrap_batch) on ONE batch -- ensembles of
1, 3, 5, 8, 0 and 67 traces (the 4-trace unroll tail of the accumulation, an empty ensemble, more than 64 traces) from h_first[0] = 2 in an
array with ld = N + 5 -- and ONE count matrix of 17 rows whose first M rows are the case M (a row does not depend on the other rows, so the
expected rows of tests/boot_batch_ref.py are computed once per frame and weight mode and shared):
  row 0, rows 6 .. 16   drawn (tspws_bootstrap_plan_batch after abi.srand)
  row 1                 all zero (K = 0: zero rows, count 0)
  row 2                 a single count of 1 (the K = 1 rule)
  row 3                 all of K on one trace: count 5 on trace 0
  row 4                 drawn, with a count of 255 on the ensemble's last trace
  row 5                 all ones
Outputs hold NaN (counts: 99) before every call: an unwritten row fails.
As a program, argv[1] = "budget", argv[2] = an .npz path: the Morlet N = 2048 batch with M = 17 under the TSPWS_PART_MB of the environment (the
library reads it once per process); with the smallest budget the call must take several rounds (102 plane pairs of 8160 coefficients are
27 MB), and the rows are written to argv[2] for the parent to compare.  Prints BOOT_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import boot_batch_ref as bbr

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")

SIZES, FIRST0, PAD, MMAX = [1, 3, 5, 8, 0, 67], 2, 5, 17
FIRST = np.concatenate([[FIRST0], FIRST0 + np.cumsum(SIZES)]).astype(np.int64)
FRAMES = {"morlet2048": (dict(), 2048), "morlet1501": (dict(), 1501), "mexhat2048": (dict(type=-3), 2048)}
WEIGHTS = {"biased": dict(wu=2.0), "unbiased": dict(wu=2.0, unbiased=1), "wu1.5": dict(wu=1.5)}
ROW_ZERO, ROW_ONE, ROW_FIVE, ROW_255, ROW_ONES = 1, 2, 3, 4, 5

_counts, _traces, _stacks, _expected, _plans = [], {}, {}, {}, {}


def counts():
    """The count matrix [17][84] (uint8) of the module's batch."""
    if not _counts:
        abi.srand(41)
        cnt = tspws.bootstrap_counts_batch(FIRST, MMAX)
        c0 = 0
        for mb in SIZES:
            if mb:
                cnt[ROW_ZERO, c0:c0 + mb] = 0
                cnt[ROW_ONE, c0:c0 + mb] = 0
                cnt[ROW_ONE, c0 + min(2, mb - 1)] = 1
                cnt[ROW_FIVE, c0:c0 + mb] = 0
                cnt[ROW_FIVE, c0] = 5
                cnt[ROW_255, c0 + mb - 1] = 255
                cnt[ROW_ONES, c0:c0 + mb] = 1
            c0 += mb
        _counts.append(cnt)
    return _counts[0]


def traces(frame):
    N = FRAMES[frame][1]
    if N not in _traces:
        _traces[N] = abi.synth_traces(int(FIRST[-1]), N, seed=N + 84)
    return _traces[N]


def params(frame, weight, **more):
    kw, N = FRAMES[frame]
    return tspws.resolve(abi.default_params(**kw, **WEIGHTS[weight], **more), N)


def expected(frame, weight):
    """Expected ls[B][17][N], ts[B][17][N], K[B][17] of the module's batch (computed once; do not modify)."""
    if (frame, weight) not in _expected:
        _expected[frame, weight] = bbr.expected(params(frame, weight), traces(frame), FIRST, counts(), _stacks.setdefault(frame, {}))
    return _expected[frame, weight]


def run(torch, frame, weight, cnt, stats=False):
    """One batched call on the padded device array; outputs held NaN (counts: 99) before it."""
    N = FRAMES[frame][1]
    if (frame, weight) not in _plans:
        X = traces(frame)
        buf = torch.zeros((X.shape[0], N + PAD), dtype=torch.float32, device="cuda")
        buf[:, :N] = torch.from_numpy(X).cuda()
        _plans[frame, weight] = (tspws.Plan(params(frame, weight), N), buf)
    pl, buf = _plans[frame, weight]
    r = dict(pl=pl, buf=buf, N=N, cnt=np.ascontiguousarray(cnt), frame=frame, weight=weight, want_stats=stats)
    return call(torch, r)


def call(torch, r):
    """The batched call of `r` (again) on NaN-filled outputs."""
    B, M, N = len(SIZES), r["cnt"].shape[0], r["N"]
    nan = float("nan")
    sl = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    st = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    sm = np.full((B, M), 99, np.uint32)
    out = r["pl"].bootstrap_batch(r["buf"][:, :N], FIRST, r["cnt"], sl, st, sm, stats=r["want_stats"])
    torch.cuda.synchronize()
    assert out[0] is sl and out[1] is st and out[2] is sm and len(out) == (4 if r["want_stats"] else 3)
    r.update(sl=sl.cpu().numpy(), st=st.cpu().numpy(), sm=sm, stats=r["pl"].bootstrap_batch_stats(), mom=out[3].cpu().numpy() if r["want_stats"] else None)
    return r


def check_counts(r):
    """What every case shares: every row written, the counts are the row sums, empty ensembles and K = 0 rows are exactly zero."""
    for k in ("sl", "st"):
        assert np.isfinite(r[k]).all(), f"{k}: rows the call did not write (NaN)"
    c0 = 0
    for b, mb in enumerate(SIZES):
        K = r["cnt"][:, c0:c0 + mb].astype(np.int64).sum(axis=1)
        np.testing.assert_array_equal(r["sm"][b], K)
        for m in np.flatnonzero(K == 0):
            assert not (r["sl"][b, m] != 0).any() and not (r["st"][b, m] != 0).any(), (b, m)
        c0 += mb


def check(r):
    """Worst relerr of the rows of `r` (the first M rows of counts()) against tests/boot_batch_ref.py; prints every ensemble's figure."""
    M = r["cnt"].shape[0]
    assert np.array_equal(r["cnt"], counts()[:M])
    check_counts(r)
    wl, wt, wk = expected(r["frame"], r["weight"])
    np.testing.assert_array_equal(r["sm"], wk[:, :M])
    worst = 0.0
    for b, mb in enumerate(SIZES):
        eb = 0.0
        for m in range(M):
            if not wk[b, m]:
                continue
            assert np.abs(wl[b, m]).max() > 0 and np.abs(wt[b, m]).max() > 0, (b, m)  # (the comparison is not between two zero rows)
            el, et = abi.relerr(r["sl"][b, m], wl[b, m]), abi.relerr(r["st"][b, m], wt[b, m])
            assert np.isfinite(el) and np.isfinite(et), (b, m)
            eb = max(eb, el, et)
        print(f"  ensemble {b} ({mb} traces): worst relerr {eb:.3e}")
        worst = max(worst, eb)
    return worst


if __name__ == "__main__":
    import torch

    if sys.argv[1] != "budget":
        raise SystemExit(f"unknown mode {sys.argv[1]}")
    r = run(torch, "morlet2048", "biased", counts())
    check_counts(r)
    st = r["stats"]
    assert st["shared"] == 5 and st["empty"] == 1 and st["rows"] == 5 * MMAX and st["max_count"] == 255, st
    np.savez(sys.argv[2], sl=r["sl"], st=r["st"], sm=r["sm"], rounds=st["rounds"])
    print("BOOT_DONE", st["rounds"], flush=True)
