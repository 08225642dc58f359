#!/usr/bin/env python3
"""Times the two-stage jackknife of many ensembles in one call (Plan.jackknife_batch_two_stage -> tspws_hip_jackknife_batch_two_stage: plain
stacks + all replicas) against the loop of Plan.stack_jackknife per ensemble, in one process, on HBM-resident traces; prints one JSON line per
shape and a last summary line.

Shapes (B x (M x N), Morlet defaults, TwoStage = 10, unbiased, delete-d jackknife over n = 12 day-of-year bins): 1000 x (30 x 4096) d = 1,
100 x (365 x 4001) d = 1 and d = 2 (C = 66: 5 column tiles), 20 x (499 x 16 501) d = 1.  Start times are drawn over one year per ensemble.
Milliseconds per batch: mean, min and max of 3 calls after one warm-up call.  Every output is filled with NaN between the two routes, and the
worst relerr of any row (plain stack or replica) between them is printed.
usage: jk_batch2_bench.py
jk_batch2_bench.py --profile: ONE batched call of 1000 x (30 x 4096), d = 1, after one warm-up call (under rocprofv3).
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
    pl = tspws.Plan(tspws.resolve(abi.default_params(Kmax=10, unbiased=1), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    rng = np.random.default_rng(7)
    year = 1420070400  # 1 Jan 2015
    times = np.concatenate([np.sort(year + rng.integers(0, 365 * 86400, m)) for m in sizes]).astype(np.int64)
    sel = tspws.jackknife_selection_batch(times, first, n, d)
    return pl, first, X, sel


def rowerr(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return max(abi.relerr(a[r], b[r]) for r in range(a.shape[0]))


if profile:
    pl, first, X, sel = setup([30] * 1000, 4096, 12, 1)
    for _ in range(2):
        pl.jackknife_batch_two_stage(X, first, sel)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="jk_batch2_bench", profile="1000 x (30 x 4096) n = 12 d = 1", stats=pl.jackknife_batch_two_stage_stats())))
    sys.exit(0)

SHAPES = [
    ("1000 x (30 x 4096) n=12 d=1", [30] * 1000, 4096, 12, 1),
    ("100 x (365 x 4001) n=12 d=1", [365] * 100, 4001, 12, 1),
    ("100 x (365 x 4001) n=12 d=2", [365] * 100, 4001, 12, 2),
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
    outs = [None] * B

    def nanfill():
        for t in (ls, ts, jl, jt):
            t.fill_(float("nan"))
        jm.fill(99)

    def loop():
        for b in range(B):
            outs[b] = pl.stack_jackknife(X[first[b]:first[b + 1]], sels[b], ls[b], ts[b])

    def batched():
        pl.jackknife_batch_two_stage(X, first, sel, ls, ts, jl, jt, jm)

    nanfill()
    t_loop = timed(loop)
    want = [ls.cpu().numpy(), ts.cpu().numpy(), np.stack([o[2].cpu().numpy() for o in outs]), np.stack([o[3].cpu().numpy() for o in outs]),
            np.stack([o[4] for o in outs])]
    outs = [None] * B
    nanfill()  # (a row the batched call does not write stays NaN and fails the comparison)
    t_batch = timed(batched)
    got = [t.cpu().numpy() for t in (ls, ts, jl, jt)]
    assert all(np.isfinite(g).all() for g in got) and np.array_equal(jm, want[4]) and jm.all(), name
    err = max(rowerr(g, w) for g, w in zip(got, want))
    r = dict(shape=name, B=B, C=Cn, traces=int(first[-1]), N=N, loop_ms=round(t_loop[0], 3), loop_min=round(t_loop[1], 3), loop_max=round(t_loop[2], 3),
             batch_ms=round(t_batch[0], 3), batch_min=round(t_batch[1], 3), batch_max=round(t_batch[2], 3), speedup=round(t_loop[0] / t_batch[0], 2),
             batch_mean_below_loop_min=bool(t_batch[0] < t_loop[1]), relerr_vs_loop=float(f"{err:.2e}"), stats=pl.jackknife_batch_two_stage_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, ls, ts, jl, jt, want, got
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="jk_batch2_bench", reps=REPS, device=torch.cuda.get_device_name(0), slowest_speedup=min(r["speedup"] for r in rows))))
