#!/usr/bin/env python3
"""Times the convergence curves of many ensembles in one call (Plan.convergence_batch -> tspws_hip_convergence_batch) against a loop of
Plan.convergence over the same ensembles, in one process, on HBM-resident traces; prints one JSON line per shape and a last summary line.

Shapes (B x (M x N), Morlet defaults): 1000 x (30 x 4096) single-stage and with TwoStage = 10, both with the step arrays, and
100 x (365 x 4001) single-stage without them.  The references are the rows of Plan.stack_batch (every ensemble against its own final stacks).
Milliseconds per batch: `reps` timed calls after one warm-up call, mean and the spread (min .. max) of the repeats, loop and batched call in the
same process.  The binding fills the batched curves and step arrays with NaN before the call: every entry must come back written, and equal to
the loop's to the bounds of the tests (similarities 1e-9 absolute, misfits 1e-7 max|loop| + 1e-18, step arrays 2e-6 relative per row).
usage: conv_batch_bench.py [reps]
conv_batch_bench.py --profile: ONE batched call of 1000 x (30 x 4096) TwoStage 10 after one warm-up call (under rocprofv3).
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not profile else 3


def timed(fn):
    """(result of the last call, [ms of every timed call]) after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def setup(sizes, N, **kw):
    pl = tspws.Plan(tspws.resolve(abi.default_params(**kw), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    ls, ts = pl.stack_batch(X, first)
    return pl, first, X, ls, ts


if profile:
    pl, first, X, ls, ts = setup([30] * 1000, 4096, Kmax=10)
    for _ in range(2):
        pl.convergence_batch(X, first, ts, ls, steps=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="conv_batch_bench", profile="1000 x (30 x 4096) TwoStage 10, two calls", stats=pl.convergence_batch_stats())))
    sys.exit(0)


def row_relerr(a, b):
    """worst max|a - b| / max|b| over the rows of two [T][N] cuda tensors (a NaN anywhere gives NaN)"""
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


SHAPES = [
    ("1000 x (30 x 4096)", [30] * 1000, 4096, {}, True),
    ("1000 x (30 x 4096) TwoStage 10", [30] * 1000, 4096, dict(Kmax=10), True),
    ("100 x (365 x 4001) no steps", [365] * 100, 4001, {}, False),
]
rows = []
for name, sizes, N, kw, steps in SHAPES:
    pl, first, X, ls, ts = setup(sizes, N, **kw)

    def loop():
        return [pl.convergence(X[first[b]:first[b + 1]], ts[b], ls[b], steps=steps) for b in range(len(sizes))]

    def batched():
        return pl.convergence_batch(X, first, ts, ls, steps=steps)

    ref, t_loop = timed(loop)
    got, t_batch = timed(batched)
    ok = True
    figures = {}
    for k, key in enumerate(("ts_sim", "ts_misfit", "ls_sim", "ls_misfit")):
        want = np.concatenate([r[k] for r in ref])
        err = float(np.max(np.abs(got[k] - want))) if np.isfinite(got[k]).all() else float("nan")
        bound = 1e-9 if key.endswith("sim") else 1e-7 * float(np.max(np.abs(want))) + 1e-18
        figures[key + "_abs_err"] = float(f"{err:.2e}")
        ok = ok and err <= bound
    if steps:
        for k, key in ((4, "ts_steps"), (5, "ls_steps")):
            err = row_relerr(got[k], torch.cat([r[k] for r in ref]))
            figures[key + "_row_relerr"] = float(f"{err:.2e}")
            ok = ok and err < 2e-6
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    # the batched call gains when even its slowest repeat beats the loop's fastest one
    r = dict(shape=name, B=len(sizes), traces=int(first[-1]), N=N, steps=steps, loop_ms=round(mean(t_loop), 3),
             loop_spread_ms=[round(min(t_loop), 3), round(max(t_loop), 3)], batch_ms=round(mean(t_batch), 3),
             batch_spread_ms=[round(min(t_batch), 3), round(max(t_batch), 3)], speedup=round(mean(t_loop) / mean(t_batch), 2),
             gains=bool(max(t_batch) < min(t_loop)), equal_to_loop=bool(ok), **figures, stats=pl.convergence_batch_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, ls, ts, ref, got
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="conv_batch_bench", reps=reps, device=torch.cuda.get_device_name(0), all_equal=all(r["equal_to_loop"] for r in rows),
                      slowest_speedup=min(r["speedup"] for r in rows))))
sys.exit(0 if all(r["equal_to_loop"] for r in rows) else 1)
