#!/usr/bin/env python3
"""Times the single-stage jackknife of many ensembles in one call (Plan.jackknife_batch -> tspws_hip_jackknife_batch: main stacks + all
replicas) against the loop of Plan.stack_single + Plan.jackknife_single per ensemble, in one process, on HBM-resident traces; prints one JSON
line per shape and a last summary line.

Shapes (B x (M x N), Morlet defaults, delete-d jackknife over n day-of-year bins): 100 x (365 x 4001) with n = 12 and d = 1 and 2,
1000 x (30 x 4096) with n = 4, d = 1, 20 x (499 x 16 501) with n = 12, d = 1.  Start times are drawn over one year per ensemble.  Milliseconds
per batch: mean, min and max of 3 calls after one warm-up call.  Every output is filled with NaN between the two routes, and the worst relerr
of any row (main or replica) between them is printed, with the padding factor of the shared pass (64-lane slots per trace).
usage: jk_batch_bench.py
jk_batch_bench.py --profile: ONE batched call of 100 x (365 x 4001), n = 12, d = 1, after one warm-up call (under rocprofv3).
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


def setup(sizes, N, n, d):
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    rng = np.random.default_rng(7)
    year = 1420070400  # 1 Jan 2015
    times = np.concatenate([np.sort(year + rng.integers(0, 365 * 86400, m)) for m in sizes]).astype(np.int64)
    sel = tspws.jackknife_selection_batch(times, first, n, d)
    return pl, first, X, sel


def padding(first, sel):
    """64-lane slots of the shared pass per trace: every (ensemble, class) starts a fresh 64-trace block."""
    slots = 0
    for b in range(len(first) - 1):
        cls, _ = tspws.selection_classes(sel[:, first[b]:first[b + 1]])
        slots += int(((np.bincount(cls) + 63) // 64).sum()) * 64
    return slots / max(1, int(first[-1]))


def rowerr(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return max(abi.relerr(a[r], b[r]) for r in range(a.shape[0]))


if profile:
    pl, first, X, sel = setup([365] * 100, 4001, 12, 1)
    for _ in range(2):
        pl.jackknife_batch(X, first, sel)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="jk_batch_bench", profile="100 x (365 x 4001) n = 12 d = 1", stats=pl.jackknife_batch_stats())))
    sys.exit(0)

SHAPES = [
    ("100 x (365 x 4001) n=12 d=1", [365] * 100, 4001, 12, 1),
    ("100 x (365 x 4001) n=12 d=2", [365] * 100, 4001, 12, 2),
    ("1000 x (30 x 4096) n=4 d=1", [30] * 1000, 4096, 4, 1),
    ("20 x (499 x 16501) n=12 d=1", [499] * 20, 16501, 12, 1),
]
rows = []
for name, sizes, N, n, d in SHAPES:
    pl, first, X, sel = setup(sizes, N, n, d)
    B, Cn = len(sizes), sel.shape[0]
    ls = torch.empty((B, N), dtype=torch.float32, device="cuda")
    ts = torch.empty_like(ls)
    jl = torch.empty((B, Cn, N), dtype=torch.float32, device="cuda")
    jt = torch.empty_like(jl)
    jm = np.zeros((B, Cn), np.uint32)
    sels = [np.ascontiguousarray(sel[:, first[b]:first[b + 1]]) for b in range(B)]

    def nanfill():
        for t in (ls, ts, jl, jt):
            t.fill_(float("nan"))
        jm.fill(99)

    def loop():
        for b in range(B):
            seg = X[first[b]:first[b + 1]]
            pl.stack_single(seg, ls[b], ts[b])
            pl.jackknife_single(seg, sels[b], jl[b], jt[b], jm[b])

    def batched():
        pl.jackknife_batch(X, first, sel, ls, ts, jl, jt, jm)

    nanfill()
    t_loop = timed(loop)
    want = [t.cpu().numpy() for t in (ls, ts, jl, jt)] + [jm.copy()]
    nanfill()  # (a row the batched call does not write stays NaN and fails the comparison)
    t_batch = timed(batched)
    got = [t.cpu().numpy() for t in (ls, ts, jl, jt)]
    assert all(np.isfinite(g).all() for g in got) and np.array_equal(jm, want[4]), name
    err = max(rowerr(g, w) for g, w in zip(got, want))
    r = dict(shape=name, B=B, C=Cn, traces=int(first[-1]), N=N, loop_ms=round(t_loop[0], 3), loop_min=round(t_loop[1], 3), loop_max=round(t_loop[2], 3),
             batch_ms=round(t_batch[0], 3), batch_min=round(t_batch[1], 3), batch_max=round(t_batch[2], 3), speedup=round(t_loop[0] / t_batch[0], 2),
             batch_mean_below_loop_min=bool(t_batch[0] < t_loop[1]), slots_per_trace=round(padding(first, sel), 2),
             relerr_vs_loop=float(f"{err:.2e}"), stats=pl.jackknife_batch_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, ls, ts, jl, jt, want, got
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="jk_batch_bench", reps=REPS, device=torch.cuda.get_device_name(0), slowest_speedup=min(r["speedup"] for r in rows))))
