#!/usr/bin/env python3
"""Times the percentile bands over replica rows (Plan.replica_bands -> tspws_hip_replica_bands) against what a user does without them, in one
process on HBM-resident rows; prints one JSON line per shape, one for the bands of a real bootstrap and a last summary line.

Routes:  (a) Plan.replica_bands;
         (b) a torch user: torch.sort(dim=1) over the rows, then a gather of x_(j), x_(j+1) and the FP64 lerp on the device;
         (c) a C or numpy user: the rows to the host, np.quantile along the replica axis there.
Shapes B x M x N (seeded normals, every replica takes part, q = 0.025, 0.5, 0.975): 8 x 100 x 16501, 32 x 100 x 16501, 8 x 100 x 131072 and
32 x 1000 x 16501 (M above lds_max_rows: the route through global memory; reported, not gated).  Milliseconds per call: mean, min and max of
3 calls per route after one warm-up call each, the routes alternating.  Every output is filled with NaN before each route's last call;
(a) and (b) must be the same floats (up to the sign of zero), (c) interpolates in float32 and must agree to 1e-5 relative.  Also: the
algorithmic bytes 4 B (M + Q) N and the fraction of the 8 TB/s HBM peak they are of (a)'s mean time.
Last: Plan.bootstrap_batch at 8 x (499 x 16501), M = 100, and the two band calls (ls, ts with its counts) on the rows it leaves.
usage: replica_bands_bench.py
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
REPS, QS, HBM_PEAK = 3, [0.025, 0.5, 0.975], 8e12
NAN = float("nan")


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(t):
    return dict(ms=round(sum(t) / len(t), 4), min=round(min(t), 4), max=round(max(t), 4))


SHAPES = [(8, 100, 16501, True), (32, 100, 16501, True), (8, 100, 131072, True), (32, 1000, 16501, False)]
lines = []
for B, M, N, gated in SHAPES:
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    rows = torch.randn((B, M, N), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B + M + N))
    Q = len(QS)
    oa = torch.empty((B, Q, N), dtype=torch.float32, device="cuda")
    ob = torch.empty_like(oa)
    oc = np.empty((B, Q, N), np.float32)
    jg = [(int(np.floor((M - 1) * q)), float((M - 1) * q - np.floor((M - 1) * q))) for q in QS]

    def route_a():
        pl.replica_bands(rows, QS, None, out=oa)

    def route_b():
        srt, _ = torch.sort(rows, dim=1)
        for k, (j, g) in enumerate(jg):
            x0 = srt[:, j].double()
            ob[:, k] = x0 if g == 0 else (x0 + g * (srt[:, j + 1].double() - x0)).float()

    def route_c():
        oc[...] = np.quantile(rows.cpu().numpy(), QS, axis=1).transpose(1, 0, 2)

    routes = (("a", route_a), ("b", route_b), ("c", route_c))
    for _, fn in routes:
        once(fn)
    t = {k: [] for k, _ in routes}
    for rep in range(REPS):
        if rep == REPS - 1:
            oa.fill_(NAN)
            ob.fill_(NAN)
            oc.fill(NAN)
        for k, fn in routes:
            t[k].append(once(fn))
    a, b = oa.cpu().numpy(), ob.cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b), (B, M, N)
    assert np.allclose(oc, a, rtol=1e-5, atol=1e-7), (B, M, N, float(np.abs(oc - a).max()))
    nbytes = 4 * B * (M + Q) * N
    r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, Q=Q, gated=gated, bands=stat(t["a"]), torch_sort=stat(t["b"]), host_quantile=stat(t["c"]),
             bands_max_below_torch_min=bool(max(t["a"]) < min(t["b"])), bands_max_below_host_min=bool(max(t["a"]) < min(t["c"])),
             a_equals_b=True, c_max_abs_diff=float(f"{np.abs(oc - a).max():.2e}"), alg_bytes=nbytes,
             hbm_peak_fraction=round(nbytes / HBM_PEAK / (sum(t["a"]) / REPS * 1e-3), 4), pcie_floor_ms=round(4 * B * M * N / 56e9 * 1e3, 3),
             stats=pl.replica_bands_stats())
    lines.append(r)
    print(json.dumps(r), flush=True)
    del pl, rows, oa, ob
    torch.cuda.empty_cache()

# the bands of a real bootstrap, next to the call that produced the rows
B, Mb, N, M = 8, 499, 16501, 100
pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
first = np.arange(B + 1, dtype=np.int64) * Mb
X = tspws.synth(B * Mb, N, seed=1)
abi.srand(1)
cnt = tspws.bootstrap_counts_batch(first, M)
sl = torch.empty((B, M, N), dtype=torch.float32, device="cuda")
st = torch.empty_like(sl)
sm = np.zeros((B, M), np.uint32)
bl = torch.empty((B, len(QS), N), dtype=torch.float32, device="cuda")
bt = torch.empty_like(bl)


def boot():
    pl.bootstrap_batch(X, first, cnt, sl, st, sm)


def bands():
    pl.replica_bands(sl, QS, sm, out=bl)
    pl.replica_bands(st, QS, sm, out=bt)


once(boot)
once(bands)
tb, tq = [once(boot) for _ in range(REPS)], [once(bands) for _ in range(REPS)]
assert bool(torch.isfinite(bl).all()) and bool(torch.isfinite(bt).all()) and bool((bl[:, 0] <= bl[:, 2]).all()) and bool((bt[:, 0] <= bt[:, 2]).all())
print(json.dumps(dict(shape="8 x (499 x 16501), M = 100", bootstrap_batch=stat(tb), two_band_calls=stat(tq), stats=pl.replica_bands_stats())), flush=True)
ok = all(r["bands_max_below_torch_min"] and r["bands_max_below_host_min"] for r in lines if r["gated"])
print(json.dumps(dict(tool="replica_bands_bench", reps=REPS, device=torch.cuda.get_device_name(0), bands_slowest_below_others_fastest_at_M100=ok)))
