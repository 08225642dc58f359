#!/usr/bin/env python3
"""Times the random subsampling of many ensembles in one call (Plan.subsample_batch -> tspws_hip_subsample_batch_sel) against the loop of
Plan.subsample_sel per ensemble with the same masks, in one process, on HBM-resident traces; prints one JSON line per shape and a last
summary line.

Shapes (B x (M_b x N), Morlet defaults, M = 8 masks, p = 0.5): 1000 x (30 x 4096), 100 x (365 x 4001) and 20 x (499 x 16 501), each
single-stage (no TwoStage) and two-stage (TwoStage = 10, unbiased).  The masks come from subsampling_selection_batch after srand(1).
Milliseconds per batch: mean, min and max of 3 calls after one warm-up call.  Every output is filled with NaN between the two routes, and the
worst relerr of any row between them is printed.
usage: sub_batch_bench.py
sub_batch_bench.py --profile: ONE batched call of 1000 x (30 x 4096), single-stage, after one warm-up call (under rocprofv3).
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
REPS, M, PROB = 3, 8, 0.5
KINDS = {"single-stage": dict(), "two-stage": dict(Kmax=10, unbiased=1)}


def timed(fn):
    """(mean, min, max) ms of REPS calls after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sum(t) / len(t), min(t), max(t)


def setup(sizes, N, kind):
    pl = tspws.Plan(tspws.resolve(abi.default_params(subsmpl_N=M, subsmpl_p=PROB, **KINDS[kind]), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    abi.srand(1)
    sel = tspws.subsampling_selection_batch(first, M, PROB)
    return pl, first, X, sel


def rowerr(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return max(abi.relerr(a[r], b[r]) for r in range(a.shape[0]))


if profile:
    pl, first, X, sel = setup([30] * 1000, 4096, "single-stage")
    for _ in range(2):
        pl.subsample_batch(X, first, sel)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="sub_batch_bench", profile="1000 x (30 x 4096) M = 8 p = 0.5 single-stage", stats=pl.subsample_batch_stats())))
    sys.exit(0)

SHAPES = [
    ("1000 x (30 x 4096)", [30] * 1000, 4096),
    ("100 x (365 x 4001)", [365] * 100, 4001),
    ("20 x (499 x 16501)", [499] * 20, 16501),
]
rows = []
for name, sizes, N in SHAPES:
    for kind in KINDS:
        pl, first, X, sel = setup(sizes, N, kind)
        B = len(sizes)
        sl = torch.empty((B, M, N), dtype=torch.float32, device="cuda")
        st = torch.empty_like(sl)
        sm = np.zeros((B, M), np.uint32)
        sels = [np.ascontiguousarray(sel[:, first[b]:first[b + 1]]) for b in range(B)]

        def nanfill():
            sl.fill_(float("nan"))
            st.fill_(float("nan"))
            sm.fill(99)

        def loop():
            for b in range(B):
                pl.subsample_sel(X[first[b]:first[b + 1]], sels[b], ls_out=sl[b], ts_out=st[b])

        def batched():
            pl.subsample_batch(X, first, sel, sl, st, sm)

        nanfill()
        t_loop = timed(loop)
        want = [sl.cpu().numpy(), st.cpu().numpy()]
        nanfill()  # (a row the batched call does not write stays NaN and fails the comparison)
        t_batch = timed(batched)
        got = [sl.cpu().numpy(), st.cpu().numpy()]
        assert all(np.isfinite(g).all() for g in got) and (sm == (sizes[0] + 1) // 2).all(), name
        err = max(rowerr(g, w) for g, w in zip(got, want))
        r = dict(shape=f"{name} {kind}", B=B, M=M, traces=int(first[-1]), N=N, loop_ms=round(t_loop[0], 3), loop_min=round(t_loop[1], 3),
                 loop_max=round(t_loop[2], 3), batch_ms=round(t_batch[0], 3), batch_min=round(t_batch[1], 3), batch_max=round(t_batch[2], 3),
                 speedup=round(t_loop[0] / t_batch[0], 2), batch_mean_below_loop_min=bool(t_batch[0] < t_loop[1]), relerr_vs_loop=float(f"{err:.2e}"),
                 stats=pl.subsample_batch_stats())
        rows.append(r)
        print(json.dumps(r), flush=True)
        del pl, X, sl, st, want, got
        torch.cuda.empty_cache()
print(json.dumps(dict(tool="sub_batch_bench", reps=REPS, device=torch.cuda.get_device_name(0), slowest_speedup=min(r["speedup"] for r in rows))))
