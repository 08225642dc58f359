#!/usr/bin/env python3
"""Times the stack's coherence filter per trace (Plan.filter_traces -> tspws_hip_filter_traces) against what a user composes without it,
in one process on HBM-resident traces; prints one JSON line per (shape, loo) and a last summary line, and writes them to
profiles/filter_traces_bench.txt (--out).

Routes:  (a) Plan.filter_traces into a given output;
         (b) the composition available before the call, ensemble by ensemble: Plan.forward, then torch FP64 / complex128 kernels for the
             phasors (zeros skipped), PS and W (leave-one-out: W per trace from PS - u_i and K - 1), then Plan.inverse, then .float();
         (c) the floor of a C caller who weights on the host: the coefficient sets to the host at the 56 GB/s of DESIGN section 6
             (computed, not run);
         (f) the transforms alone, ensemble by ensemble: Plan.forward and Plan.inverse on the unweighted sets (the same
             tspws_hip_forward_f32 / tspws_hip_inverse calls, into NaN-filled tensors);
         (k) the weighting alone: Plan.filter_coef on ONE ensemble's sets, out of place (k_cf_weight for one ensemble, one table upload and
             k_cf_apply: 16 + 16 bytes per coefficient and row), times B, next to
         (p) the yardstick of an HBM-streaming pass on this device in this run: the partial-stack pass (tspws_hip_partial_stacks) over the
             same traces, 4 bytes per trace sample.
Shapes B x (M x N): 8 x (499 x 16501) and 32 x (499 x 16501), default Morlet frame, wu = 2, biased, single-stage; loo = 0 and 1.
Milliseconds per call from device events: the median (min .. max) of REPS calls per route after one warm-up each, the routes alternating.
(a) and (b) are compared per row at the parity tolerance.  No PMC counters are collected here.
usage: filter_traces_bench.py [--reps R] [--shape I] [--out PATH]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import abi

tspws = importlib.import_module("ts-pws_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shape", type=int, default=-1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_traces_bench.txt"))
args = ap.parse_args()
REPS, PCIE = max(args.reps, 1), 56e9
lines = []


def emit(r):
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)


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


SHAPES = [(8, 499, 16501), (32, 499, 16501)]
for idx, (B, M, N) in enumerate(SHAPES):
    if args.shape >= 0 and idx != args.shape:
        continue
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    nc = pl.ncoef
    first = np.arange(B + 1, dtype=np.int64) * M
    X = tspws.synth(B * M, N, seed=11)
    K1 = np.array([M], np.uint32)
    ens0 = np.zeros(M, np.uint32)
    Pk = 8
    P = torch.empty((Pk, N), dtype=torch.float64, device="cuda")
    out_a = torch.empty((B * M, N), dtype=torch.float32, device="cuda")
    out_b = torch.empty((B * M, N), dtype=torch.float32, device="cuda")
    Y0 = pl.forward(X[:M])
    PS0 = torch.where(Y0 != 0, Y0 / Y0.abs(), torch.zeros_like(Y0)).sum(0, keepdim=True).contiguous()
    out_k = torch.empty_like(Y0)
    for loo in (False, True):
        def route_a():
            pl.filter_traces(X, first, loo=loo, out=out_a)

        def route_b():
            for b in range(B):
                Y = pl.forward(X[b * M:(b + 1) * M])
                mag = Y.abs()
                u = torch.where(mag > 0, Y / mag, torch.zeros_like(Y))
                PS = u.sum(0)
                if loo:
                    W = ((PS[None, :] - u).abs() / (M - 1)) ** 2
                else:
                    W = ((PS.abs() / M) ** 2)[None, :]
                out_b[b * M:(b + 1) * M] = pl.inverse((Y * W).contiguous()).float()
                del Y, mag, u, PS, W

        def route_f():
            for b in range(B):
                pl.inverse(pl.forward(X[b * M:(b + 1) * M]))

        def route_k():
            pl.filter_coef(Y0, PS0, K1, ens=ens0, loo=loo, out=out_k)

        def route_p():
            tspws.check(pl.lib.tspws_hip_partial_stacks(pl.h, X.data_ptr(), N, B * M, 0, B * M, Pk, P.data_ptr(), N, pl._stream()), "partial_stacks")

        routes = (("a", route_a), ("b", route_b), ("f", route_f), ("k", route_k), ("p", route_p))
        for _, fn in routes:
            timed(fn)
        t = {k: [] for k, _ in routes}
        for rep in range(REPS):
            if rep == REPS - 1:
                out_a.fill_(float("nan"))
                out_b.fill_(float("nan"))
            for k, fn in routes:
                t[k].append(timed(fn))
        route_a()
        stats = pl.filter_traces_stats()
        top = out_b.abs().amax(dim=1)
        rel = float(((out_a - out_b).abs().amax(dim=1) / top).max())
        assert bool(torch.isfinite(out_a).all()) and rel < 2e-6, rel
        med = {k: float(np.median(v)) for k, v in t.items()}
        coef_bytes = 16 * B * M * nc
        k_bytes, p_bytes = 32 * M * nc, 4 * B * M * N
        k_rate, p_rate = k_bytes / (med["k"] * 1e-3), p_bytes / (med["p"] * 1e-3)
        emit(dict(shape=f"{B} x ({M} x {N})", B=B, M=M, N=N, loo=int(loo), S=pl.S, ncoef=nc, filter_traces_ms=stat(t["a"]), composed_torch_ms=stat(t["b"]),
                  pcie_floor_ms=round(coef_bytes / PCIE * 1e3, 3), coefficient_bytes=coef_bytes, transforms_only_ms=stat(t["f"]),
                  weighting_one_ensemble_ms=stat(t["k"]), weighting_all_ms=round(med["k"] * B, 4), weighting_share_of_call=round(med["k"] * B / med["a"], 3),
                  transforms_share_of_call=round(med["f"] / med["a"], 3), composed_over_call=round(med["b"] / med["a"], 2),
                  a_max_below_b_min=bool(max(t["a"]) < min(t["b"])), k_cf_apply_bytes=k_bytes, k_cf_apply_TBps=round(k_rate / 1e12, 3),
                  partial_stacks_ms=stat(t["p"]), partial_stacks_TBps=round(p_rate / 1e12, 3), k_cf_apply_fraction_of_partial_stacks_rate=round(k_rate / p_rate, 3),
                  max_rel_diff_a_b=float(f"{rel:.2e}"), stats=stats))
    del pl, X, P, out_a, out_b, Y0, PS0, out_k
    torch.cuda.empty_cache()

emit(dict(tool="filter_traces_bench", reps=REPS, device=torch.cuda.get_device_name(0), pmc_counters="not collected"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
