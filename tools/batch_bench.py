#!/usr/bin/env python3
"""Times many same-length ensembles in one call (Plan.stack_batch -> tspws_hip_stack_batch) against a loop of Plan.stack_single over the same
ensembles, in one process, on HBM-resident traces; prints one JSON line per shape and a last summary line.

Shapes (B x (M x N), Morlet defaults): 1000 x (30 x 4096), 500 x (64 x 8192), 100 x (365 x 4001), 20 x (499 x 16 501), 1000 x (30 x 4096) with
TwoStage = 10, one mixed batch (sizes 5 .. 400 at N = 4096, Kmax = 10: single- and two-stage ensembles) and one single-stage batch of varied
sizes (5 .. 60 at N = 4096: many segment geometries, so many accumulation launches).  Milliseconds per batch, mean of `reps` calls after one
warm-up call; the outputs are filled with NaN between the loop and the batched calls, and the batched rows are compared with the loop's.
usage: batch_bench.py [reps]
batch_bench.py --profile: ONE batched call of 1000 x (30 x 4096) single-stage after one warm-up call (under rocprofv3).
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not profile else 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def setup(sizes, N, **kw):
    pl = tspws.Plan(tspws.resolve(abi.default_params(**kw), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    return pl, first, X


if profile:
    pl, first, X = setup([30] * 1000, 4096)
    for _ in range(2):
        pl.stack_batch(X, first)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="batch_bench", profile="1000 x (30 x 4096) single-stage")))
    sys.exit(0)

rng = np.random.default_rng(7)
SHAPES = [
    ("1000 x (30 x 4096)", [30] * 1000, 4096, {}),
    ("500 x (64 x 8192)", [64] * 500, 8192, {}),
    ("100 x (365 x 4001)", [365] * 100, 4001, {}),
    ("20 x (499 x 16501)", [499] * 20, 16501, {}),
    ("1000 x (30 x 4096) TwoStage 10", [30] * 1000, 4096, dict(Kmax=10)),
    ("mixed 300 x (5..400 x 4096) TwoStage 10", list(rng.integers(5, 401, 300)), 4096, dict(Kmax=10)),
    ("varied 1000 x (5..60 x 4096) single-stage", list(rng.integers(5, 61, 1000)), 4096, {}),
]
rows = []
for name, sizes, N, kw in SHAPES:
    pl, first, X = setup(sizes, N, **kw)
    ls = torch.empty((len(sizes), N), dtype=torch.float32, device="cuda")
    ts = torch.empty_like(ls)

    def loop():
        for b in range(len(sizes)):
            pl.stack_single(X[first[b]:first[b + 1]], ls[b], ts[b])

    def batched():
        pl.stack_batch(X, first, ls, ts)

    t_loop = timed(loop)
    ref_ls, ref_ts = ls.clone(), ts.clone()
    ls.fill_(float("nan"))
    ts.fill_(float("nan"))  # (a row the batched call did not write stays NaN and fails the comparison)
    t_batch = timed(batched)
    got_ls, got_ts = ls.cpu().numpy(), ts.cpu().numpy()
    assert np.isfinite(got_ls).all() and np.isfinite(got_ts).all(), name
    err = max(abi.relerr(got_ls, ref_ls.cpu().numpy()), abi.relerr(got_ts, ref_ts.cpu().numpy()))
    r = dict(shape=name, B=len(sizes), traces=int(first[-1]), N=N, loop_ms=round(t_loop, 3), batch_ms=round(t_batch, 3),
             speedup=round(t_loop / t_batch, 2), relerr_vs_loop=float(f"{err:.2e}"), stats=pl.batch_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, ls, ts, ref_ls, ref_ts
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="batch_bench", reps=reps, device=torch.cuda.get_device_name(0),
                      slowest_speedup=min(r["speedup"] for r in rows))))
