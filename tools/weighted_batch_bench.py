#!/usr/bin/env python3
"""Times the real-weighted stacks of many ensembles in one call (Plan.weighted_stack_batch -> tspws_hip_weighted_stack_batch) next to the
counted call on the same rows (Plan.bootstrap_batch -> tspws_hip_bootstrap_batch_cnt, without the statistics) -- in one process, on
HBM-resident traces; prints one JSON line per shape and a last summary line.  The rows are integer weights drawn as bootstrap counts
(bootstrap_counts_batch after srand(1)): the one kind of row both calls take.  The weighted call multiplies where the counted one adds
repeatedly, so it is expected not to be slower than the counted call beyond that call's own spread; the counted call is therefore timed
TWICE (columns boot_a, boot_b), the three routes alternating.

Shapes (B x (M_b x N), Morlet defaults, single-stage): 8 and 32 ensembles of 499 x 16 501 with M = 8 and M = 100 rows.  Milliseconds per batch:
mean, min and max of 3 calls per route after one warm-up call each.  Every output is filled with NaN before each route's last call, and the
worst relerr of any row between the two calls is printed (biased weights: the two estimators agree to rounding).
usage: weighted_batch_bench.py
weighted_batch_bench.py --profile: ONE call of each kind on 8 x (499 x 16501), M = 100, after one warm-up call each (under rocprofv3
--kernel-trace --stats: the times of k_rb_accumulate<WeightRows> and k_rb_accumulate<CountRows> side by side).
"""
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import abi

tspws = importlib.import_module("ts-pws_amd")
profile = len(sys.argv) > 1 and sys.argv[1] == "--profile"
REPS = 3


def once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def setup(sizes, N, M):
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    abi.srand(1)
    cnt = tspws.bootstrap_counts_batch(first, M)
    return pl, first, X, cnt, cnt.astype(np.float64)


def rowerr(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return max(abi.relerr(a[r], b[r]) for r in range(a.shape[0]))


if profile:
    pl, first, X, cnt, w = setup([499] * 8, 16501, 100)
    for _ in range(2):
        pl.bootstrap_batch(X, first, cnt)
        pl.weighted_stack_batch(X, first, w)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="weighted_batch_bench", profile="8 x (499 x 16501) M = 100", stats=pl.weighted_stack_batch_stats())))
    sys.exit(0)

SHAPES = [(f"{B} x (499 x 16501) M = {M}", [499] * B, 16501, M) for B in (8, 32) for M in (8, 100)]
rows = []
for name, sizes, N, M in SHAPES:
    pl, first, X, cnt, w = setup(sizes, N, M)
    B = len(sizes)
    sl = torch.empty((B, M, N), dtype=torch.float32, device="cuda")
    st = torch.empty_like(sl)
    sm = np.zeros((B, M), np.uint32)

    def nanfill():
        sl.fill_(float("nan"))
        st.fill_(float("nan"))
        sm.fill(99)

    def counted():
        pl.bootstrap_batch(X, first, cnt, sl, st, sm)

    def weighted():
        pl.weighted_stack_batch(X, first, w, sl, st, sm)

    once(counted)
    once(weighted)
    t_a, t_w, t_b = [], [], []
    for rep in range(REPS):
        last = rep == REPS - 1
        t_a.append(once(counted))
        if last:
            nanfill()
        t_w.append(once(weighted))
        if last:
            got = [sl.cpu().numpy(), st.cpu().numpy()]
            assert (sm == (cnt > 0).reshape(M, B, sizes[0]).sum(axis=2).T).all(), name
            nanfill()  # (a row the next call does not write stays NaN and fails the comparison)
        t_b.append(once(counted))
    want = [sl.cpu().numpy(), st.cpu().numpy()]
    assert all(np.isfinite(g).all() for g in got + want) and (sm == sizes[0]).all(), name
    err = max(rowerr(g, x) for g, x in zip(got, want))
    ma, mw, mb = sum(t_a) / REPS, sum(t_w) / REPS, sum(t_b) / REPS
    r = dict(shape=name, B=B, M=M, traces=int(first[-1]), N=N, weighted_ms=round(mw, 3), weighted_min=round(min(t_w), 3), weighted_max=round(max(t_w), 3),
             boot_a_ms=round(ma, 3), boot_a_min=round(min(t_a), 3), boot_a_max=round(max(t_a), 3), boot_b_ms=round(mb, 3), boot_b_min=round(min(t_b), 3),
             boot_b_max=round(max(t_b), 3), weighted_over_boot=round(mw / (0.5 * (ma + mb)), 3), boot_spread=round(max(t_a + t_b) / min(t_a + t_b), 3),
             weighted_max_within_boot_max=bool(max(t_w) <= max(t_a + t_b)), relerr_vs_boot=float(f"{err:.2e}"), max_count=int(cnt.max()),
             stats=pl.weighted_stack_batch_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, sl, st, want, got
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="weighted_batch_bench", reps=REPS, device=torch.cuda.get_device_name(0), worst_weighted_over_boot=max(r["weighted_over_boot"] for r in rows))))
