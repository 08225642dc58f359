#!/usr/bin/env python3
"""Times dv/v per band from the wavelet cross-spectrum (Plan.wxs_rows -> tspws_hip_wxs_rows) against what a user does without it, in one
process on HBM-resident rows; prints one JSON line per shape and a last summary line.

Routes:  (a) Plan.wxs_rows with the sums wanted;
         (b) a torch user: per ensemble Plan.forward on its rows and its reference, then the cross-spectrum, abs, angle and the nine terms as
             torch elementwise kernels in FP64 and one FP64 matmul per window against the 0 / 1 matrix of (coefficient in window and band);
         (c) the floor of a C caller without the call: the coefficient sets to the host at the 56 GB/s of DESIGN section 6 (computed, not run).
The call is also split: (f) the forward transforms alone (Plan.forward: the same tspws_hip_forward_f32 calls, into NaN-filled tensors) and (r)
the reduction alone (Plan.wxs_coef on the sets that (f) left).  Where all sets are below 4 GB both take all rows at once; otherwise (f) goes
ensemble by ensemble and (r) takes the sets of ONE ensemble, times B.  (p) is the yardstick of a read-once kernel, not a competitor: the
streaming partial-stack pass (tspws_hip_partial_stacks, 8 groups) over the float rows of the same run, in bytes per second.
Shapes B x M x N: 8 x 100 x 16501 and 32 x 1000 x 16501 (seeded normals; every row takes part), the frame's decimation octaves as bands,
W = 2: the coda windows of lags 500 .. 6000 samples on either side of z = 8250.  Milliseconds per call from device events: the median
(min .. max) of REPS calls per route after one warm-up each, the routes alternating.  (a) and (b) are compared on the sums.  The reduction's
bytes: 32 per coefficient inside a window and a band (16 of the row's set, 16 of the reference's; the reference's are shared by the M rows of
an ensemble and mostly come from cache, so the HBM figure counts the row's 16 only).
usage: wxs_rows_bench.py [--reps R] [--shape I]      (--shape: only shape I, for a kernel-trace run)
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shape", type=int, default=-1)
args = ap.parse_args()
REPS, PCIE = max(args.reps, 1), 56e9
NAN = float("nan")
Z, WINS = 8250.0, ((2250, 7751), (8750, 14251))  # lags 500 .. 6000 inclusive on either side


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
    tb = pl.tables()
    D, Ns, S = tb["D"].astype(np.int64), tb["Ns"].astype(np.int64), pl.S
    edges = [0] + [s for s in range(1, S) if D[s] != D[s - 1]] + [S]
    bands = list(zip(edges[:-1], edges[1:]))
    R, W = len(bands), len(WINS)
    gen = torch.Generator(device="cuda").manual_seed(B + M + N)
    ref = torch.randn((B, N), dtype=torch.float32, device="cuda", generator=gen)
    rows = ref[:, None, :] + 0.5 * torch.randn((B, M, N), dtype=torch.float32, device="cuda", generator=gen)
    # per coefficient: scale, sample position, 1 / omega; per window the 0 / 1 matrix [ncoef][R]
    sc = np.repeat(np.arange(S), Ns)
    pos = np.concatenate([np.arange(n) * d for n, d in zip(Ns, D)]).astype(np.float64)
    omega = pl.info.w0 / tb["scale"]
    t_c = torch.from_numpy(pos - Z).cuda()
    om_c = torch.from_numpy(omega[sc]).cuda()
    G = np.zeros((W, pl.ncoef, R))
    for w, (n0, n1) in enumerate(WINS):
        for r, (s0, s1) in enumerate(bands):
            G[w, :, r] = (sc >= s0) & (sc < s1) & (pos >= n0) & (pos < n1)
    inwin = int(sum(((pos >= n0) & (pos < n1)).sum() for n0, n1 in WINS))
    G = torch.from_numpy(G).cuda()
    a_sums = torch.empty((B, M, W, R, 9), dtype=torch.float64, device="cuda")
    a_fit = torch.empty((B, M, W, R, 6), dtype=torch.float64, device="cuda")
    b_sums = torch.empty_like(a_sums)
    keep = {}

    def route_a():
        pl.wxs_rows(rows, ref, Z, bands, WINS, sums=True, out=(a_sums, a_fit))

    whole = 16 * (B * M + B) * pl.ncoef < 4 << 30
    r_sums, r_fit = (torch.empty_like(a_sums), torch.empty_like(a_fit)) if whole else (torch.empty_like(a_sums[0]), torch.empty_like(a_fit[0]))
    ens = np.arange(B * M, dtype=np.uint32) // M if whole else np.zeros(M, np.uint32)
    P = torch.empty((8, N), dtype=torch.float64, device="cuda")

    def route_f():
        if whole:
            keep["Yc"], keep["Yr"] = pl.forward(rows.view(B * M, N)), pl.forward(ref)
            return
        for b in range(B):
            keep["Yc"], keep["Yr"] = pl.forward(rows[b]), pl.forward(ref[b:b + 1])

    def route_r():
        pl.wxs_coef(keep["Yc"], keep["Yr"], Z, bands, WINS, ens=ens, sums=True, out=(r_sums, r_fit))

    def route_p():
        tspws.check(pl.lib.tspws_hip_partial_stacks(pl.h, rows.data_ptr(), N, B * M, 0, B * M, 8, P.data_ptr(), N, pl._stream()), "partial_stacks")

    def route_b():
        for b in range(B):
            Yc, Yr = pl.forward(rows[b]), pl.forward(ref[b:b + 1])
            X = Yc * Yr.conj()
            a = X.abs()
            ok = torch.isfinite(a) & (a > 0)
            a = torch.where(ok, a, 0.0)
            delta = X.angle() / om_c
            at, ad = a * t_c, a * delta
            terms = torch.stack([ok.double(), a, at, at * t_c, ad, at * delta, ad * delta, torch.where(ok, X.real, 0.0), torch.where(ok, X.imag, 0.0)], dim=1)
            del X, a, ok, delta, at, ad
            for w in range(W):
                b_sums[b, :, w] = torch.matmul(terms, G[w]).transpose(1, 2)  # [M][9][R] -> [M][R][9]
            del terms

    routes = (("a", route_a), ("f", route_f), ("r", route_r), ("b", route_b), ("p", route_p))
    for _, fn in routes:
        timed(fn)
    t = {k: [] for k, _ in routes}
    for rep in range(REPS):
        if rep == REPS - 1:
            a_sums.fill_(NAN)
            a_fit.fill_(NAN)
            b_sums.fill_(NAN)
        for k, fn in routes:
            t[k].append(timed(fn))
        if rep == REPS - 1:
            assert bool(torch.isfinite(a_sums).all()) and bool(torch.isfinite(b_sums).all()), (B, M, N)
            scale = b_sums.abs().amax(dim=(0, 1, 2, 3))
            diff = float(((a_sums - b_sums).abs().amax(dim=(0, 1, 2, 3)) / scale).max())
    route_a()
    stats = pl.wxs_rows_stats()
    assert diff < 1e-9, diff
    if whole:
        assert torch.equal(r_sums, a_sums) and torch.equal(r_fit, a_fit)  # the reduction alone on the same sets: the call's own bits
    coef_bytes = 16 * (B * M + B) * pl.ncoef
    floor = coef_bytes / PCIE * 1e3
    red_ms = float(np.median(t["r"])) * (1 if whole else B)
    ps_ms = float(np.median(t["p"]))
    r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, ncoef=pl.ncoef, bands=R, windows=WINS, wxs_rows_ms=stat(t["a"]), torch_fp64_ms=stat(t["b"]),
             forward_only_ms=stat(t["f"]), reduce_ms=stat(t["r"]), reduce_covers="all rows" if whole else "one ensemble", reduce_all_ms=round(red_ms, 4), pcie_floor_ms=round(floor, 3),
             coefficient_bytes=coef_bytes, a_max_below_b_min=bool(max(t["a"]) < min(t["b"])), a_max_below_pcie_floor=bool(max(t["a"]) < floor),
             sums_max_rel_diff_a_b=float(f"{diff:.2e}"), coefficients_in_windows_per_row=inwin,
             reduce_row_set_GBps=round(16 * inwin * B * M / (red_ms * 1e-3) / 1e9, 1), reduce_both_sets_GBps=round(32 * inwin * B * M / (red_ms * 1e-3) / 1e9, 1),
             partial_stacks_ms=stat(t["p"]), partial_stacks_GBps=round(4 * B * M * N / (ps_ms * 1e-3) / 1e9, 1), stats=stats)
    lines.append(r)
    print(json.dumps(r), flush=True)
    del pl, rows, ref, a_sums, a_fit, b_sums, r_sums, r_fit, G, keep
    torch.cuda.empty_cache()

print(json.dumps(dict(tool="wxs_rows_bench", reps=REPS, device=torch.cuda.get_device_name(0))))
