#!/usr/bin/env python3
"""Times the single-stage jackknife (tspws_hip_jackknife_single) on HBM-resident traces and prints ONE JSON line.

Shapes 499 x 16 501 and 1024 x 32 768, single stage (Morlet defaults), start times over one year, n = 12 with d = 1, 2, 3 (C = 12, 66,
220).  Per case: the plain single-stage stack (plain_ms), the replicas alone (jk_ms), the stack followed by the replicas -- what
tspws_main runs (stack_jk_ms) --, and the masked-accumulation route on the same masks as the baseline (tspws_hip_subsample_sel,
masked_ms).  Milliseconds per call, mean of `reps` calls after one warm-up call.   usage: jk_single_bench.py [reps]
jk_single_bench.py --profile D: ONE stack + replicas call at 499 x 16 501, n = 12, d = D, after one warm-up call (under rocprofv3).
"""
import ctypes as C
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
lib = tspws.load()
profile_d = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--profile" else 0
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not profile_d else 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


if profile_d:
    N = 16501
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    X = tspws.synth(499, N, seed=1)
    sel = tspws.jackknife_selection(np.sort(1420070400 + np.random.default_rng(499).integers(0, 365 * 86400, 499)).astype(np.int64), 12, profile_d)
    for _ in range(2):
        pl.stack_single(X)
        pl.jackknife_single(X, sel)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="jk_single_bench", profile_d=profile_d, C=sel.shape[0])))
    sys.exit(0)

rows = []
for mtr, N in ((499, 16501), (1024, 32768)):
    p = tspws.resolve(abi.default_params(), N)
    pl = tspws.Plan(p, N)
    X = tspws.synth(mtr, N, seed=1)
    rng = np.random.default_rng(mtr)
    times = np.sort(1420070400 + rng.integers(0, 365 * 86400, mtr)).astype(np.int64)  # 2015
    plain = timed(lambda: pl.stack_single(X))
    for d in (1, 2, 3):
        sel = tspws.jackknife_selection(times, 12, d)
        Cn = sel.shape[0]
        jl = torch.empty((Cn, N), dtype=torch.float32, device="cuda")
        jt = torch.empty((Cn, N), dtype=torch.float32, device="cuda")
        jm = np.zeros(Cn, np.uint32)
        jk = timed(lambda: pl.jackknife_single(X, sel, jl, jt, jm))
        both = timed(lambda: (pl.stack_single(X), pl.jackknife_single(X, sel, jl, jt, jm)))
        q = tspws.t_tsPWS.from_buffer_copy(pl.params)
        q.subsmpl_p = (int(jm[0]) - 0.5) / mtr  # (K of every mask = replica 0's; the time does not depend on it)
        ml = torch.empty((Cn, N), dtype=torch.float32, device="cuda")
        mt = torch.empty((Cn, N), dtype=torch.float32, device="cuda")
        masked = timed(lambda: tspws.check(lib.tspws_hip_subsample_sel(pl.h, C.byref(q), X.data_ptr(), N, mtr, Cn, sel.ctypes.data, ml.data_ptr(),
                                                                      mt.data_ptr(), None), "subsample_sel"))
        # (sanity: replica 0 of both routes)
        err0 = abi.relerr(jt[0].cpu().numpy(), mt[0].cpu().numpy())
        rows.append(dict(mtr=mtr, N=N, n=12, d=d, C=Cn, plain_ms=round(plain, 3), jk_ms=round(jk, 3), stack_jk_ms=round(both, 3),
                         masked_ms=round(masked, 3), replica0_relerr_vs_masked=err0))
    pl.close()
print(json.dumps(dict(tool="jk_single_bench", device=torch.cuda.get_device_name(0), reps=reps, cases=rows)))
