#!/usr/bin/env python3
"""Times dv/v by dynamic time warping (Plan.dtw_rows -> tspws_hip_dtw_rows) against what a user does without it, in one process on
HBM-resident rows; prints one JSON line per (shape, parameter set), one for the lone wave and a last summary line.

Routes:  (a) Plan.dtw_rows (fit and lags);
         (b) a torch user: the same recurrence on the device in FP64, vectorised over all rows and lags, a python loop over the samples --
             per sample the error row, the slanted candidates from a ring of the last b accumulated rows and b - 1 error rows, the choice
             by comparisons and torch.where, the choice row kept as uint8 -- WITHOUT the backtrack and the fit.  Its cost per sample is
             constant, so it is timed over the first --torch-steps samples of each range (all of them when 0) and reported per sample and
             scaled to the ranges' length; the smallest accumulated error over those samples must equal route (a)'s dist on the same
             prefix ranges bit for bit;
         (c) the floor of a C caller without the call: the rows to the host at the 56 GB/s of DESIGN section 6 (computed, not run).
Shapes B x M x N: 8 x 100 x 16501 and 32 x 1000 x 16501 (seeded normals smoothed over 9 samples: the rows are their reference plus noise of
half its size; every row takes part), W = 2: the lag ranges 500 .. 6000 samples on either side of z = 8250 (5501 samples each), at
Lmax = 31, b = 4 and at Lmax = 127, b = 8.  Milliseconds per call from device events: the median (min .. max) of REPS calls after one
warm-up.  The lone wave: B = M = W = 1 at range lengths 5501 and 16501; the difference over 11000 samples is what one sample costs a wave
that has the machine to itself (forward and backward), in ns and in cycles at the 2.4 GHz of DESIGN section 6.
usage: dtw_rows_bench.py [--reps R] [--shape I] [--torch-steps S] [--torch-steps-large S]
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
ap.add_argument("--torch-steps", type=int, default=512)
ap.add_argument("--torch-steps-large", type=int, default=64)
args = ap.parse_args()
REPS, PCIE, GHZ = max(args.reps, 1), 56e9, 2.4
Z, RANGES = 8250.0, ((2250, 7751), (8750, 14251))  # lags 500 .. 6000 inclusive on either side
SETS = (dict(Lmax=31, b=4), dict(Lmax=127, b=8))
INF = float("inf")


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


def torch_forward(rows, ref, n0, steps, Lmax, b):
    """The accumulation over the samples n0 .. n0 + steps - 1 of rows [R][N] against ref [R][N] (ensemble-expanded): (D_end [R][nl], the
    uint8 choice rows).  The normalisation uses the maxima over this prefix range, as the call on the prefix range does."""
    R, N = rows.shape
    nl = 2 * Lmax + 1
    k0, k1 = max(0, n0 - Lmax), min(N, n0 + steps + Lmax)
    ac = 1.0 / rows[:, n0:n0 + steps].abs().amax(dim=1).double()
    ar = 1.0 / ref[:, k0:k1].abs().amax(dim=1).double()
    lags = torch.arange(-Lmax, Lmax + 1, device=rows.device)
    inf = torch.full((R, 1), INF, dtype=torch.float64, device=rows.device)
    Dring, Ering, choices = [], [], []
    for i in range(steps):
        idx = (n0 + i + lags).clamp(0, N - 1)
        d = (rows[:, n0 + i].double() * ac)[:, None] - ref[:, idx].double() * ar[:, None]
        e = d * d
        if i == 0:
            D = e
        else:
            ib = max(0, i - b)
            V = Dring[ib - i]
            for k in range(i - 1, ib, -1):
                V = V + Ering[k - i]
            dc = Dring[-1]
            dm = torch.cat([inf, V[:, :-1]], dim=1)
            dp = torch.cat([V[:, 1:], inf], dim=1)
            isc = (dc <= dm) & (dc <= dp)
            ism = ~isc & (dm <= dp)
            D = e + torch.where(isc, dc, torch.where(ism, dm, dp))
            choices.append(torch.where(isc, 0, torch.where(ism, 1, 2)).to(torch.uint8))
        Dring = (Dring + [D])[-b:]
        Ering = (Ering + [e])[-b:]
    return D, choices


# ---- the lone wave ----
N1 = 16501
pl = tspws.Plan(tspws.resolve(abi.default_params(), N1), N1)
gen = torch.Generator(device="cuda").manual_seed(1)
ref1 = torch.randn((1, N1), dtype=torch.float32, device="cuda", generator=gen)
row1 = ref1[:, None, :] + 0.5 * torch.randn((1, 1, N1), dtype=torch.float32, device="cuda", generator=gen)
for par in SETS:
    t = {}
    for n in (5501, 16501):
        fn = lambda: pl.dtw_rows(row1, ref1, Z, par, ((0, n),))
        timed(fn)
        t[n] = [timed(fn) for _ in range(REPS)]
    ns = (float(np.median(t[16501])) - float(np.median(t[5501]))) * 1e6 / 11000
    print(json.dumps(dict(lone_wave=par, ms_5501=stat(t[5501]), ms_16501=stat(t[16501]), ns_per_sample=round(ns, 1), cycles_per_sample_at_2p4_ghz=round(ns * GHZ, 1))),
          flush=True)
del pl

SHAPES = [(8, 100, 16501), (32, 1000, 16501)]
for idx, (B, M, N) in enumerate(SHAPES):
    if args.shape >= 0 and idx != args.shape:
        continue
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    gen = torch.Generator(device="cuda").manual_seed(B + M + N)
    smooth = torch.ones((1, 1, 9), dtype=torch.float32, device="cuda") / 3
    ref = torch.nn.functional.conv1d(torch.randn((B, 1, N + 8), dtype=torch.float32, device="cuda", generator=gen), smooth)[:, 0]
    rows = ref[:, None, :] + 0.5 * torch.nn.functional.conv1d(torch.randn((B * M, 1, N + 8), dtype=torch.float32, device="cuda", generator=gen), smooth).view(B, M, N)
    steps = (args.torch_steps, args.torch_steps_large)[idx] or RANGES[0][1] - RANGES[0][0]
    steps = min(steps, RANGES[0][1] - RANGES[0][0])
    prefix = tuple((n0, n0 + steps) for n0, _ in RANGES)
    flat, refx = rows.view(B * M, N), ref[:, None, :].expand(B, M, N).reshape(B * M, N)
    for par in SETS:
        keep = {}

        def route_a():
            keep["a"] = pl.dtw_rows(rows, ref, Z, par, RANGES)

        def route_b():
            keep["b"] = [torch_forward(flat, refx, n0, steps, par["Lmax"], par["b"])[0] for n0, _ in prefix]

        timed(route_a)
        ta = [timed(route_a) for _ in range(REPS)]
        stats = pl.dtw_rows_stats()
        fit = keep["a"]["fit"]
        assert bool(torch.isfinite(fit).all()) and bool((keep["a"]["lag"].abs() <= par["Lmax"]).all()), (B, M, N)
        timed(route_b)
        tb = [timed(route_b) for _ in range(max(1, min(REPS, 3)))]
        # the torch route's smallest accumulated error against the call's dist on the same prefix ranges: bit for bit
        pfit = pl.dtw_rows(rows, ref, Z, par, prefix, lag=False)
        for w in range(2):
            assert torch.equal(keep["b"][w].amin(dim=1) / float(steps), pfit[:, :, w, 4].reshape(-1)), (par, w)
        per_step = [x / (2 * steps) for x in tb]
        full = [x * (RANGES[0][1] - RANGES[0][0]) / steps for x in tb]
        floor = 4 * B * M * N / PCIE * 1e3
        nwaves, nsteps = B * M * 2, RANGES[0][1] - RANGES[0][0]
        r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, par=par, ranges=RANGES, dtw_rows_ms=stat(ta), torch_steps_timed_per_range=steps,
                 torch_fp64_ms_per_sample=stat(per_step), torch_fp64_ms_scaled_to_the_ranges=stat(full), torch_dist_bit_equal=True, pcie_floor_ms=round(floor, 3),
                 a_max_below_b_min=bool(max(ta) < min(full)), a_max_below_pcie_floor=bool(max(ta) < floor),
                 ns_per_wave_sample_in_the_batch=round(float(np.median(ta)) * 1e6 / (nwaves * nsteps), 3), eps_hat_median=float(fit[..., 0].median()), stats=stats)
        print(json.dumps(r), flush=True)
        del keep
    del pl, rows, ref, flat, refx
    torch.cuda.empty_cache()

print(json.dumps(dict(tool="dtw_rows_bench", reps=REPS, device=torch.cuda.get_device_name(0))))
