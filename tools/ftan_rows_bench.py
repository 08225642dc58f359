#!/usr/bin/env python3
"""Times the group arrivals per scale (Plan.ftan_rows -> tspws_hip_ftan_rows) against what a user does without it, in one process on
HBM-resident rows; prints one JSON line per (shape, P) and a last summary line.

Routes:  (a) Plan.ftan_rows with the noise level wanted;
         (b) a torch user: per ensemble Plan.forward on its rows, then in FP64 torch kernels the squared modulus, the shifted compares of
             the peak rule under the window's mask, and one topk per (scale, window);
         (c) the floor of a C caller without the call: the coefficient sets to the host at the 56 GB/s of DESIGN section 6 (computed, not run).
The call is also split: (f) the forward transforms alone (Plan.forward: the same tspws_hip_forward_f32 calls, into NaN-filled tensors) and (r)
the reduction alone (Plan.ftan_coef on the sets that (f) left).  Where all sets are below 4 GB both take all rows at once; otherwise (f) goes
ensemble by ensemble and (r) takes the sets of ONE ensemble, times B.  (x) is the yardstick: the wavelet cross-spectrum's reduction
(Plan.wxs_coef, octave bands) on the same sets and windows in the same run, each in bytes of the rows' sets inside the windows per second.
Shapes B x M x N: 8 x 100 x 16501 and 32 x 1000 x 16501 (seeded normals; every row takes part), all scales, W = 2: the causal and acausal
windows of group velocities 2 .. 4.5 at distances 4000 + 250 (b % 16) (ftan_windows; dt = 1, z = 8250), so up to 16 classes of ensembles;
the noise range is the last 2000 samples.  P = 1 and 4.  Milliseconds per call from device events: the median (min .. max) of REPS calls per
route after one warm-up each, the routes alternating.  (a) and (b) are compared on the peaks' indices.
usage: ftan_rows_bench.py [--reps R] [--shape I]      (--shape: only shape I, for a kernel-trace run)
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
REPS, PCIE = max(args.reps, 1), 56e9
NAN = float("nan")
Z = 8250.0


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
for idx, (B, M, N) in enumerate(SHAPES):
    if args.shape >= 0 and idx != args.shape:
        continue
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    tb = pl.tables()
    D, Ns, S = tb["D"].astype(np.int64), tb["Ns"].astype(np.int64), pl.S
    off = np.concatenate([[0], np.cumsum(Ns)])
    wins = np.stack([tspws.ftan_windows(4000.0 + 250.0 * (b % 16), 2.0, 4.5, 1.0, Z, N, 2) for b in range(B)]).astype(np.int64)
    noise = np.array([N - 2000, N], np.int64)
    edges = [0] + [s for s in range(1, S) if D[s] != D[s - 1]] + [S]
    octaves = list(zip(edges[:-1], edges[1:]))
    gen = torch.Generator(device="cuda").manual_seed(B + M + N)
    rows = torch.randn((B, M, N), dtype=torch.float32, device="cuda", generator=gen)
    # per (ensemble, window, scale) the 0 / 1 mask of the interior indices 1 .. Ns - 2 that are members
    masks = [[[torch.from_numpy(((np.arange(1, Ns[s] - 1) * D[s] >= wins[b, w, 0]) & (np.arange(1, Ns[s] - 1) * D[s] < wins[b, w, 1]))).cuda() for s in range(S)]
              for w in range(2)] for b in range(B)]
    inwin = np.array([sum(int(((np.arange(Ns[s]) * D[s] >= wins[b, w, 0]) & (np.arange(Ns[s]) * D[s] < wins[b, w, 1])).sum()) for s in range(S) for w in range(2))
                      for b in range(B)])
    innoise = sum(int(((np.arange(Ns[s]) * D[s] >= noise[0]) & (np.arange(Ns[s]) * D[s] < noise[1])).sum()) for s in range(S))
    whole = 16 * B * M * pl.ncoef < 4 << 30
    ens = np.arange(B * M, dtype=np.uint32) // M if whole else np.zeros(M, np.uint32)
    keep = {}

    def route_f():
        if whole:
            keep["Y"] = pl.forward(rows.view(B * M, N))
            return
        for b in range(B):
            keep["Y"] = pl.forward(rows[b])

    for P in (1, 4):
        a_peaks = torch.empty((B, M, 2, S, P, 5), dtype=torch.float64, device="cuda")
        a_noise = torch.empty((B, M, S, 2), dtype=torch.float64, device="cuda")
        b_k = torch.empty((B, M, 2, S, P), dtype=torch.int64, device="cuda")
        r_peaks, r_noise = (torch.empty_like(a_peaks), torch.empty_like(a_noise)) if whole else (torch.empty_like(a_peaks[0]), torch.empty_like(a_noise[0]))

        def route_a():
            pl.ftan_rows(rows, Z, wins, P=P, noise=noise, out=(a_peaks, a_noise))

        def route_r():
            pl.ftan_coef(keep["Y"], Z, wins if whole else wins[B - 1:], P=P, noise=noise, ens=ens, B=B if whole else 1, out=(r_peaks, r_noise))

        def route_x():
            pl.wxs_coef(keep["Y"], keep["Y"][:B if whole else 1], Z, octaves, wins[B - 1], ens=ens, out=keep["x_fit"])

        def route_b():
            for b in range(B):
                Y = pl.forward(rows[b])
                a2 = Y.real * Y.real + Y.imag * Y.imag
                for s in range(S):
                    a = a2[:, off[s]:off[s + 1]]
                    mid = a[:, 1:-1]
                    pk = (mid > a[:, :-2]) & (mid >= a[:, 2:]) & torch.isfinite(a[:, :-2]) & torch.isfinite(mid) & torch.isfinite(a[:, 2:])
                    for w in range(2):
                        v = torch.where(pk & masks[b][w][s], mid, -1.0)
                        if v.shape[1] < P:
                            v = torch.nn.functional.pad(v, (0, P - v.shape[1]), value=-1.0)
                        val, at = torch.topk(v, P, dim=1)
                        b_k[b, :, w, s] = torch.where(val > 0, at + 1, -1)
                del Y, a2

        keep["x_fit"] = torch.empty(((B * M if whole else M), 2, len(octaves), 6), dtype=torch.float64, device="cuda")
        routes = (("a", route_a), ("f", route_f), ("r", route_r), ("x", route_x), ("b", route_b))
        for _, fn in routes:
            timed(fn)
        t = {k: [] for k, _ in routes}
        for rep in range(REPS):
            if rep == REPS - 1:
                a_peaks.fill_(NAN)
                b_k.fill_(-7)
            for k, fn in routes:
                t[k].append(timed(fn))
        a_k = a_peaks[..., 4].long()
        differ = int((a_k != b_k).sum())
        assert differ == 0, differ  # (seeded normals: no two peaks of a scale share their a2)
        route_a()
        stats = pl.ftan_rows_stats()
        if whole:
            assert torch.equal(r_peaks.view(torch.int64), a_peaks.view(torch.int64)) and torch.equal(r_noise, a_noise)  # the reduction alone: the call's own bits
        coef_bytes = 16 * B * M * pl.ncoef
        floor = coef_bytes / PCIE * 1e3
        mult = 1 if whole else B
        red_ms, wx_ms = float(np.median(t["r"])) * mult, float(np.median(t["x"])) * mult
        ft_bytes = 16 * M * (float(inwin.sum()) + B * innoise) if whole else 16 * M * B * float(inwin[B - 1] + innoise)
        wx_bytes = 16 * M * B * float(inwin[B - 1])
        r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, P=P, S=S, ncoef=pl.ncoef, ftan_rows_ms=stat(t["a"]), torch_fp64_ms=stat(t["b"]), forward_only_ms=stat(t["f"]),
                 reduce_ms=stat(t["r"]), reduce_covers="all rows" if whole else "one ensemble", reduce_all_ms=round(red_ms, 4),
                 reduce_share_of_call=round(red_ms / float(np.median(t["a"])), 3), pcie_floor_ms=round(floor, 3), coefficient_bytes=coef_bytes,
                 a_max_below_b_min=bool(max(t["a"]) < min(t["b"])), a_max_below_pcie_floor=bool(max(t["a"]) < floor), peak_indices_that_differ_a_b=differ, peak_slots=a_k.numel(),
                 coefficients_in_windows_per_row=int(inwin[B - 1]), coefficients_in_noise_range_per_row=innoise,
                 ftan_reduce_GBps=round(ft_bytes / (red_ms * 1e-3) / 1e9, 1), wxs_reduce_ms=stat(t["x"]), wxs_reduce_all_ms=round(wx_ms, 4),
                 wxs_reduce_row_set_GBps=round(wx_bytes / (wx_ms * 1e-3) / 1e9, 1), stats=stats)
        print(json.dumps(r), flush=True)
        del a_peaks, a_noise, b_k, r_peaks, r_noise
    del pl, rows, masks, keep
    torch.cuda.empty_cache()

print(json.dumps(dict(tool="ftan_rows_bench", reps=REPS, device=torch.cuda.get_device_name(0))))
