#!/usr/bin/env python3
"""Times dv/v by the moving-window cross-spectrum (Plan.mwcs_rows -> tspws_hip_mwcs_rows) against what a user does without it, in one
process on HBM-resident rows; prints one JSON line per shape and a last summary line.

Routes:  (a) Plan.mwcs_rows;
         (b) a torch user, ensemble by ensemble: unfold the lag ranges into windows, FP64 demean and taper, torch.fft.rfft of length P,
             the band's bins, the cross-spectrum and powers, the smoothing as one matmul with the normalised kernel matrix, coherence,
             phase, the weighted regression over the bins and the two regressions over the windows, all as torch kernels;
         (c) the floor of a C caller without the call: the rows to the host at the 56 GB/s of DESIGN section 6 (computed, not run).
Shapes B x M x N: 8 x 100 x 16501 and 32 x 1000 x 16501 (seeded normals: the rows are their reference plus noise of half its size; every
row takes part), L = 512, hop = 128, P = 512, the 32 bins [20, 52), h = 4, taper 0.15, no filter, W = 2: the lag ranges 500 .. 6000 samples
on either side of z = 8250.  Milliseconds per call from device events: the median (min .. max) of REPS calls per route after one warm-up
each, the routes alternating; the outputs are NaN-filled before the last call.  (a) and (b) are compared on d_fit.  The contraction's
FLOP count: 2 x (rows + references) x J x L x 2 Qx.
usage: mwcs_rows_bench.py [--reps R] [--shape I]      (--shape: only shape I, for a kernel-trace run)
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
Z, RANGES = 8250.0, ((2250, 7751), (8750, 14251))  # lags 500 .. 6000 inclusive on either side
PAR = dict(L=512, hop=128, P=512, q0=20, q1=52, h=4, taper=0.15, min_coh=0.0, max_err=float("inf"), max_delta=float("inf"), err_floor=1e-3)


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


par = tspws.mwcs_par(**PAR)
tab = tspws.mwcs_basis(par)
qa, qb, Qx = tspws.mwcs_qrange(par)
L, hop, P, h, nq, lo = par.L, par.hop, par.P, par.h, par.q1 - par.q0, par.q0 - qa
wins = tspws.mwcs_windows(par, RANGES)
J, W = wins.shape[0], len(RANGES)
g = torch.from_numpy(tab["g"]).cuda()
v = torch.from_numpy(tab["v"][lo:lo + nq]).cuda()
# the smoothing as a [Qx][nq] matrix: column q holds k[d] / sum of the same k[d] at rows q + d inside [0, Qx)
Ksm = np.zeros((Qx, nq))
for q in range(nq):
    ds = [d for d in range(-h, h + 1) if 0 <= lo + q + d < Qx]
    for d in ds:
        Ksm[lo + q + d, q] = tab["k"][d + h] / sum(tab["k"][e + h] for e in ds)
Ksm = torch.from_numpy(Ksm).cuda()
t_j = torch.from_numpy((wins[:, 0].astype(np.float64) + 0.5 * (L - 1)) - Z).cuda()

SHAPES = [(8, 100, 16501), (32, 1000, 16501)]
for idx, (B, M, N) in enumerate(SHAPES):
    if args.shape >= 0 and idx != args.shape:
        continue
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    gen = torch.Generator(device="cuda").manual_seed(B + M + N)
    ref = torch.randn((B, N), dtype=torch.float32, device="cuda", generator=gen)
    rows = ref[:, None, :] + 0.5 * torch.randn((B, M, N), dtype=torch.float32, device="cuda", generator=gen)
    b_fit = torch.empty((B, M, W, 6), dtype=torch.float64, device="cuda")
    keep = {}

    def spectra(x):
        """float32 [..][N] -> complex128 [..][J][Qx]"""
        fr = torch.cat([x[..., n0:n1].unfold(-1, L, hop) for n0, n1 in RANGES], dim=-2).double()
        fr = (fr - fr.mean(dim=-1, keepdim=True)) * g
        return torch.fft.rfft(fr, n=P, dim=-1)[..., qa:qb]

    def route_a():
        keep["a"] = pl.mwcs_rows(rows, ref, Z, par, RANGES)

    def route_b():
        for b in range(B):
            Fc, Fr = spectra(rows[b]), spectra(ref[b])
            X = Fc * Fr.conj()
            sX = torch.complex(X.real @ Ksm, X.imag @ Ksm)
            sPc, sPr = (Fc.real ** 2 + Fc.imag ** 2) @ Ksm, (Fr.real ** 2 + Fr.imag ** 2) @ Ksm
            a = sX.abs()
            coh = a / torch.sqrt(sPc * sPr)
            phi = sX.angle()
            c2 = coh.clamp(max=0.99) ** 2
            wv = torch.sqrt(c2 / (1 - c2) * torch.sqrt(a)) * v
            svv = (wv * v).sum(-1)
            delta = (wv * phi).sum(-1) / svv
            s2 = ((phi - delta[..., None] * v) ** 2).sum(-1) / (nq - 1)
            err = torch.sqrt((wv * wv).sum(-1) * s2) / svv
            p = 1.0 / err.clamp(min=PAR["err_floor"]) ** 2
            for w in range(W):
                js = slice(int((wins[:, 1] < w).sum()), int((wins[:, 1] <= w).sum()))
                pw, t, d = p[:, js], t_j[js], delta[:, js]
                S, St, Stt, Sd, Std = pw.sum(-1), (pw * t).sum(-1), (pw * t * t).sum(-1), (pw * d).sum(-1), (pw * t * d).sum(-1)
                den = S * Stt - St * St
                b_fit[b, :, w] = torch.stack([(S * Std - St * Sd) / den, (Stt * Sd - St * Std) / den, torch.sqrt(S / den), Std / Stt, torch.sqrt(1 / Stt),
                                              torch.full_like(S, js.stop - js.start)], dim=-1)

    routes = (("a", route_a), ("b", route_b))
    for _, fn in routes:
        timed(fn)
    t = {k: [] for k, _ in routes}
    for rep in range(REPS):
        if rep == REPS - 1:
            b_fit.fill_(NAN)   # (route a returns outputs of its own, NaN-filled before every call)
        for k, fn in routes:
            t[k].append(timed(fn))
    a_fit = keep["a"]
    assert bool(torch.isfinite(a_fit).all()) and bool(torch.isfinite(b_fit).all()), (B, M, N)
    assert torch.equal(a_fit[..., 5], b_fit[..., 5])
    scale = b_fit.abs().amax(dim=(0, 1, 2))
    diff = (a_fit - b_fit).abs().amax(dim=(0, 1, 2)) / scale
    stats = pl.mwcs_rows_stats()
    assert float(diff.max()) < 1e-6, diff
    floor = 4 * B * M * N / PCIE * 1e3
    flop = 2.0 * (B * M + B) * J * L * 2 * Qx
    r = dict(shape=f"{B} x {M} x {N}", B=B, M=M, N=N, par={k: (x if np.isfinite(x) else "inf") for k, x in PAR.items()}, ranges=RANGES, J=J, Qx=Qx,
             mwcs_rows_ms=stat(t["a"]), torch_fp64_ms=stat(t["b"]), pcie_floor_ms=round(floor, 3), a_max_below_b_min=bool(max(t["a"]) < min(t["b"])),
             a_max_below_pcie_floor=bool(max(t["a"]) < floor), fit_max_rel_diff_a_b=[float(f"{x:.2e}") for x in diff.tolist()],
             contraction_gflop=round(flop / 1e9, 3), stats=stats)
    print(json.dumps(r), flush=True)
    del pl, rows, ref, b_fit, keep
    torch.cuda.empty_cache()

print(json.dumps(dict(tool="mwcs_rows_bench", reps=REPS, device=torch.cuda.get_device_name(0))))
