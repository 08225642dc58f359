#!/usr/bin/env python3
"""Times the band rows on HBM-resident data with HIP events on the stream; prints one JSON line per shape and a last summary line.
  (a) tspws_hip_inverse_bands with the quadrature: the R band rows X_r, Q_r of every set from ONE pass over the sets;
  (b) what the library offered before for the same rows: per band, a masked copy and a rotated (-i) masked copy of the sets through
      tspws_hip_inverse (the masking on the device, the band's coefficient range only; timed with it);
      shapes of (a) against (b): 16 sets at N = 16 501 and 2 sets at N = 131 072, with R = 6 bands that partition the scales and with R = S
      (every scale a band);
  (c) tspws_hip_stack_batch_bands with R = 6 and envelopes against tspws_hip_stack_batch alone at 8 x (499 x 16 501): the price of the bands
      on top of a stack.
Milliseconds: median, min and max of 7 calls per route after 2 warm-up calls each, the routes alternating in one process.  Before the timed
calls the rows of (a) are compared with those of (b) (worst abi.relerr of a row: both are FP64 sums of the same terms).
usage: band_rows_bench.py [--profile]
--profile: two calls of each route of the first shape after one warm-up each and nothing else (for rocprofv3 --kernel-trace --stats).
"""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import abi

tspws = importlib.import_module("ts-pws_amd")
lib = tspws.load()
profile = len(sys.argv) > 1 and sys.argv[1] == "--profile"
WARM, REPS = 2, 7


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(routes):
    """{name: [ms] * REPS}: the routes one after the other, WARM + REPS times."""
    t = {k: [] for k in routes}
    for i in range(WARM + REPS):
        for k, fn in routes.items():
            ms = timed(fn)
            if i >= WARM:
                t[k].append(ms)
    return t


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def partition(S, R):
    cuts = [round(i * S / R) for i in range(R + 1)]
    return [(cuts[i], cuts[i + 1]) for i in range(R)]


def inverse_shape(nset, N, R):
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    S, nc = pl.S, pl.ncoef
    bands = partition(S, R if R else S)
    R = len(bands)
    bt = tspws.band_table(bands)
    off = np.concatenate([[0], np.cumsum(pl.tables()["Ns"].astype(np.int64))])
    g = torch.Generator(device="cuda").manual_seed(7)
    Y = torch.view_as_complex(torch.randn((nset, nc, 2), dtype=torch.float64, device="cuda", generator=g).contiguous())
    re = torch.empty((nset, R, N), dtype=torch.float64, device="cuda")
    im = torch.empty_like(re)
    Ym = torch.zeros((2 * nset, nc), dtype=torch.complex128, device="cuda")
    xb = torch.empty((R, 2 * nset, N), dtype=torch.float64, device="cuda")

    def bands_call():
        tspws.check(lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), nset, bt.ctypes.data, R, re.data_ptr(), im.data_ptr(), stream()), "inverse_bands")

    def masked_calls():
        for r, (a, e) in enumerate(bands):
            lo, hi = int(off[a]), int(off[e])
            Ym.zero_()
            Ym[:nset, lo:hi] = Y[:, lo:hi]
            Ym[nset:, lo:hi] = Y[:, lo:hi] * (-1j)
            tspws.check(lib.tspws_hip_inverse(pl.h, Ym.data_ptr(), 2 * nset, xb[r].data_ptr(), stream()), "inverse")

    bands_call()
    masked_calls()
    torch.cuda.synchronize()
    err = max(max(abi.relerr(re[j, r].cpu().numpy(), xb[r, j].cpu().numpy()), abi.relerr(im[j, r].cpu().numpy(), xb[r, nset + j].cpu().numpy()))
              for j in range(nset) for r in range(R))
    return pl, dict(bands=bands_call, masked=masked_calls), err, S, R


if profile:
    pl, routes, err, S, R = inverse_shape(16, 16501, 6)
    for _ in range(2):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="band_rows_bench", profile="16 sets at N = 16501, R = 6", relerr=float(f"{err:.2e}"))))
    sys.exit(0)

rows = []
for nset, N in ((16, 16501), (2, 131072)):
    for R in (6, 0):
        pl, routes, err, S, R = inverse_shape(nset, N, R)
        t = alternate(routes)
        r = dict(what="inverse_bands + quadrature vs masked copies through inverse", sets=nset, N=N, S=S, R=R, bands_ms=stats(t["bands"]),
                 masked_ms=stats(t["masked"]), bands_over_masked=round(statistics.median(t["bands"]) / statistics.median(t["masked"]), 3),
                 relerr_rows=float(f"{err:.2e}"))
        rows.append(r)
        print(json.dumps(r), flush=True)
        del pl, routes
        torch.cuda.empty_cache()

# (c) the price of the bands on top of a stack
B, M, N, R = 8, 499, 16501, 6
pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
first = np.ascontiguousarray(np.arange(B + 1) * M, dtype=np.uint64)
X = tspws.synth(B * M, N, seed=1)
bt = tspws.band_table(partition(pl.S, R))
outs = [torch.empty((B, R, N), dtype=torch.float32, device="cuda") for _ in range(4)]
ls, ts = (torch.empty((B, N), dtype=torch.float32, device="cuda") for _ in range(2))


def stack_bands():
    tspws.check(lib.tspws_hip_stack_batch_bands(pl.h, C.byref(pl.params), X.data_ptr(), N, first.ctypes.data, B, bt.ctypes.data, R, *[o.data_ptr() for o in outs],
                                                stream()), "stack_batch_bands")


def stack_plain():
    tspws.check(lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), X.data_ptr(), N, first.ctypes.data, B, ls.data_ptr(), ts.data_ptr(), stream()), "stack_batch")


t = alternate(dict(bands=stack_bands, plain=stack_plain))
full = sum(outs[1][:, r].double() for r in range(R)).float().cpu().numpy()   # the R bands partition the scales
r = dict(what="stack_batch_bands (R = 6, envelopes) vs stack_batch", shape=f"{B} x ({M} x {N})", R=R, bands_ms=stats(t["bands"]), plain_ms=stats(t["plain"]),
         bands_over_plain=round(statistics.median(t["bands"]) / statistics.median(t["plain"]), 3),
         relerr_sum_of_bands_vs_ts=float(f"{max(abi.relerr(full[b], ts[b].cpu().numpy()) for b in range(B)):.2e}"), stats=pl.stack_batch_bands_stats())
rows.append(r)
print(json.dumps(r), flush=True)
print(json.dumps(dict(tool="band_rows_bench", warmups=WARM, reps=REPS, device=torch.cuda.get_device_name(0), timing="HIP events on the stream")))
