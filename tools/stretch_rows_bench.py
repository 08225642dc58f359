#!/usr/bin/env python3
"""Times dv/v by stretching (Plan.stretch_rows -> tspws_hip_stretch_rows) against what a user does without it, in one process on
HBM-resident rows; prints one JSON line per shape and a last summary line.

Routes:  (a) Plan.stretch_rows with the cc plane wanted;
         (b) a torch user: the stretched references by gathers and the cubic polynomial in FP64, then torch.bmm with rows.double() and
             the normalisation, window by window;
         (c) the floor of a C caller without the call: the rows to the host at the 56 GB/s of DESIGN section 6 (computed, not run).
Shapes B x M x N: 8 x 100 x 16501 and 32 x 1000 x 16501 (seeded normals; every row takes part), the grid stretch_grid(0.01, 201), W = 2: the
coda windows of lags 500 .. 6000 samples on either side of z = 8250.  Milliseconds per call from device events: the median (min .. max) of
REPS >= 7 calls per route after one warm-up each, the routes alternating.  Every output is filled with NaN before each route's last call;
(a) and (b) are compared on cc and the largest difference is printed.  Also the contraction's 2 B M E sum n_w flops.
usage: stretch_rows_bench.py [--reps R] [--shape I]      (--shape: only shape I, for a kernel-trace run)
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import abi

tspws = importlib.import_module("ts-pws_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shape", type=int, default=-1)
args = ap.parse_args()
REPS, FP64_PEAK, PCIE = max(args.reps, 1), 78.6e12, 56e9
NAN = float("nan")
Z, WINS, E = 8250.0, ((2250, 7751), (8750, 14251)), 201  # lags 500 .. 6000 inclusive on either side


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stat(t):
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


SHAPES = [(8, 100, 16501), (32, 1000, 16501)]
lines = []
for idx, (B, M, N) in enumerate(SHAPES):
    if args.shape >= 0 and idx != args.shape:
        continue
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    gen = torch.Generator(device="cuda").manual_seed(B + M + N)
    ref = torch.randn((B, N), dtype=torch.float32, device="cuda", generator=gen)
    rows = ref[:, None, :] + 0.5 * torch.randn((B, M, N), dtype=torch.float32, device="cuda", generator=gen)
    eps = tspws.stretch_grid(0.01, E)
    eps_t = torch.from_numpy(eps).cuda()
    W = len(WINS)
    a_cc = torch.empty((B, M, W, E), dtype=torch.float64, device="cuda")
    a_fit = torch.empty((B, M, W, 4), dtype=torch.float64, device="cuda")
    b_cc = torch.empty_like(a_cc)

    def route_a():
        pl.stretch_rows(rows, ref, Z, eps, WINS, cc=True, out=(a_cc, a_fit))

    def route_b():
        refp = torch.nn.functional.pad(ref.double(), (4, 4))  # sample j at j + 4: zeros outside [0, N)
        for w, (n0, n1) in enumerate(WINS):
            n = torch.arange(n0, n1, dtype=torch.float64, device="cuda")[None, :]
            u = n + (n - Z) * eps_t[:, None]
            fl = torch.floor(u)
            f = u - fl
            i = fl.clamp(-3, N + 1).long() + 4  # (further out all four samples are zeros)
            wk = (((-0.5 * f + 1) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1, ((-1.5 * f + 2) * f + 0.5) * f, (0.5 * f - 0.5) * f * f)
            S = sum(wk[k][None] * refp[:, i + (k - 1)] for k in range(4))  # [B][E][n]
            c = rows[:, :, n0:n1].double()
            dot = torch.bmm(c, S.transpose(1, 2))
            b_cc[:, :, w] = dot / (c * c).sum(-1).sqrt()[:, :, None] / (S * S).sum(-1).sqrt()[:, None, :]

    routes = (("a", route_a), ("b", route_b))
    for _, fn in routes:
        timed(fn)
    t = {k: [] for k, _ in routes}
    for rep in range(REPS):
        if rep == REPS - 1:
            a_cc.fill_(NAN)
            a_fit.fill_(NAN)
            b_cc.fill_(NAN)
        for k, fn in routes:
            t[k].append(timed(fn))
    assert bool(torch.isfinite(a_cc).all()) and bool(torch.isfinite(b_cc).all()) and bool(torch.isfinite(a_fit).all()), (B, M, N)
    diff = float((a_cc - b_cc).abs().max())
    assert diff < 1e-12, diff
    flops = 2 * B * M * E * sum(n1 - n0 for n0, n1 in WINS)
    floor = 4 * B * M * N / PCIE * 1e3
    r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, E=E, windows=WINS, stretch_rows_ms=stat(t["a"]), torch_fp64_ms=stat(t["b"]), pcie_floor_ms=round(floor, 3),
             a_max_below_b_min=bool(max(t["a"]) < min(t["b"])), a_max_below_pcie_floor=bool(max(t["a"]) < floor), cc_max_abs_diff_a_b=float(f"{diff:.2e}"),
             contraction_flops=flops, call_tflops=round(flops / (float(np.median(t["a"])) * 1e-3) / 1e12, 2),
             call_share_of_fp64_peak=round(flops / (float(np.median(t["a"])) * 1e-3) / FP64_PEAK, 4), stats=pl.stretch_rows_stats())
    lines.append(r)
    print(json.dumps(r), flush=True)
    del pl, rows, ref, a_cc, a_fit, b_cc
    torch.cuda.empty_cache()

ok = all((r["a_max_below_b_min"] or r["M"] != 100) and r["a_max_below_pcie_floor"] for r in lines)
print(json.dumps(dict(tool="stretch_rows_bench", reps=REPS, device=torch.cuda.get_device_name(0), required_orderings_hold=ok)))
