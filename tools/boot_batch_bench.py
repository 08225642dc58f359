#!/usr/bin/env python3
"""Times the bootstrap of many ensembles in one call (Plan.bootstrap_batch -> tspws_hip_bootstrap_batch_cnt, with the statistics) against what a
user does without it: per replica a device gather of the expanded ensemble (index_select with the replica's repeated trace indices, built
before the clock starts) and one Plan.subsample_sel with an all-ones mask and prob 1 -- in one process, on HBM-resident traces; prints one JSON
line per shape and a last summary line.

Shapes (B x (M_b x N), Morlet defaults, single-stage, M = 100 replicas): 8 and 32 ensembles of 499 x 16 501 and of 16 x 2048.  The counts come
from bootstrap_counts_batch after srand(1).  Milliseconds per batch: mean, min and max of 3 calls per route after one warm-up call each, the
routes alternating.  Every output is filled with NaN before each route's last call, and the worst relerr of any row between them is printed.
usage: boot_batch_bench.py
boot_batch_bench.py --profile: ONE batched call of 8 x (499 x 16501) after one warm-up call (under rocprofv3).
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
REPS, M = 3, 100


def once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def setup(sizes, N):
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=1)
    abi.srand(1)
    cnt = tspws.bootstrap_counts_batch(first, M)
    return pl, first, X, cnt


def rowerr(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return max(abi.relerr(a[r], b[r]) for r in range(a.shape[0]))


if profile:
    pl, first, X, cnt = setup([499] * 8, 16501)
    for _ in range(2):
        pl.bootstrap_batch(X, first, cnt, stats=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="boot_batch_bench", profile="8 x (499 x 16501) M = 100", stats=pl.bootstrap_batch_stats())))
    sys.exit(0)

SHAPES = [
    ("8 x (499 x 16501)", [499] * 8, 16501),
    ("32 x (499 x 16501)", [499] * 32, 16501),
    ("8 x (16 x 2048)", [16] * 8, 2048),
    ("32 x (16 x 2048)", [16] * 32, 2048),
]
rows = []
for name, sizes, N in SHAPES:
    pl, first, X, cnt = setup(sizes, N)
    B = len(sizes)
    sl = torch.empty((B, M, N), dtype=torch.float32, device="cuda")
    st = torch.empty_like(sl)
    sm = np.zeros((B, M), np.uint32)
    # the expanded ensembles' trace indices, per (ensemble, replica), on the device
    idx = [[torch.from_numpy(np.repeat(np.arange(sizes[b]), cnt[m, first[b]:first[b + 1]])).cuda() for m in range(M)] for b in range(B)]
    ones = [np.ones((1, sizes[b]), np.int8) for b in range(B)]

    def nanfill():
        sl.fill_(float("nan"))
        st.fill_(float("nan"))
        sm.fill(99)

    def gathered():
        for b in range(B):
            Xb = X[first[b]:first[b + 1]]
            for m in range(M):
                pl.subsample_sel(Xb.index_select(0, idx[b][m]), ones[b], prob=1.0, ls_out=sl[b, m:m + 1], ts_out=st[b, m:m + 1])

    def batched():
        pl.bootstrap_batch(X, first, cnt, sl, st, sm, stats=True)

    once(gathered)
    once(batched)
    t_loop, t_batch = [], []
    for rep in range(REPS):
        last = rep == REPS - 1
        if last:
            nanfill()
        t_loop.append(once(gathered))
        if last:
            want = [sl.cpu().numpy(), st.cpu().numpy()]
            nanfill()  # (a row the batched call does not write stays NaN and fails the comparison)
        t_batch.append(once(batched))
    got = [sl.cpu().numpy(), st.cpu().numpy()]
    assert all(np.isfinite(g).all() for g in got) and (sm == sizes[0]).all(), name
    err = max(rowerr(g, w) for g, w in zip(got, want))
    ml, mb = sum(t_loop) / REPS, sum(t_batch) / REPS
    r = dict(shape=name, B=B, M=M, traces=int(first[-1]), N=N, gather_ms=round(ml, 3), gather_min=round(min(t_loop), 3), gather_max=round(max(t_loop), 3),
             batch_ms=round(mb, 3), batch_min=round(min(t_batch), 3), batch_max=round(max(t_batch), 3), speedup=round(ml / mb, 2),
             batch_max_below_gather_min=bool(max(t_batch) < min(t_loop)), relerr_vs_gather=float(f"{err:.2e}"), stats=pl.bootstrap_batch_stats())
    rows.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, sl, st, want, got, idx
    torch.cuda.empty_cache()
print(json.dumps(dict(tool="boot_batch_bench", reps=REPS, device=torch.cuda.get_device_name(0), slowest_speedup=min(r["speedup"] for r in rows))))
