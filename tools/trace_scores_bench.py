#!/usr/bin/env python3
"""Times the trace scores (Plan.trace_scores -> tspws_hip_trace_scores, R = 2) against what a caller can do without them, in one process on
HBM-resident traces; prints one JSON line per shape and a last summary line.

Routes:  (a) Plan.trace_scores with two reference rows per ensemble;
         (b) a torch user on the device: x.double(), then products and row sums for the same four sums per reference;
         (c) the streaming partial-stack pass (tspws_hip_partial_stacks, k_partial) over the same array: not a competitor but the yardstick of
             an HBM-streaming pass on this box in this run -- its algorithmic bytes are the same 4 bytes per trace sample.
Shapes: 1 ensemble of 10 000 x 131 072 (the headline array, 5.2 GB) and 8 ensembles of 499 x 16 501 (the scalar load route: 16 501 is odd).
Synthetic traces; the references are the mean of the ensemble and the mean of its first 64 traces.  Milliseconds per call from HIP events
on the stream: the median, min and max of REPS calls per route after WARM warm-up calls each, the routes alternating.  (a) and (b) must agree
to 1e-9 relative on misfit, dot and the energy and to 1e-9 absolute on sim.  Reported: bytes/s of (a) and (c) over their algorithmic bytes
(4 bytes per trace sample of the window; (a) also reads the reference rows once per ensemble from HBM), (a)'s fraction of (c)'s rate and of
the 8 TB/s HBM peak, and the ratio of (b)'s time to (a)'s.
usage: trace_scores_bench.py
"""
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
WARM, REPS, HBM_PEAK = 2, 7, 8e12


def timed(fn):
    """Milliseconds of fn() between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(t):
    return dict(ms=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))


SHAPES = [(1, 10000, 131072, 10), (8, 499, 16501, 8)]  # ensembles, traces per ensemble, samples, groups of the partial-stack pass
lines = []
for B, M, N, K in SHAPES:
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    first = np.arange(B + 1, dtype=np.int64) * M
    X = tspws.synth(B * M, N, seed=3)
    refs = torch.stack([torch.stack([X[b * M:(b + 1) * M].mean(0), X[b * M:b * M + 64].mean(0)]) for b in range(B)]).contiguous()
    P = torch.empty((K, N), dtype=torch.float64, device="cuda")
    out = {}

    def route_a():
        out["a"] = pl.trace_scores(X, first, refs, energy=True)

    def route_b():
        xd = X.double().view(B, M, N)
        rd = refs.double()
        xx = (xd * xd).sum(2)
        planes = []
        for k in range(2):
            r = rd[:, k:k + 1]
            dot = (xd * r).sum(2)
            rr = (r * r).sum(2)
            planes.append(torch.stack([dot / xx.sqrt() / rr.sqrt(), ((xd - r) ** 2).sum(2), dot]).reshape(3, B * M))
        out["b"] = (torch.stack(planes), xx.reshape(B * M))

    def route_c():
        tspws.check(pl.lib.tspws_hip_partial_stacks(pl.h, X.data_ptr(), N, B * M, 0, B * M, K, P.data_ptr(), N, pl._stream()), "partial_stacks")

    routes = (("a", route_a), ("b", route_b), ("c", route_c))
    for _, fn in routes:
        for _ in range(WARM):
            timed(fn)
    t = {k: [] for k, _ in routes}
    for rep in range(REPS):
        for k, fn in routes:
            t[k].append(timed(fn))
    (sa, ea), (sb, eb) = out["a"], out["b"]
    assert bool(torch.isfinite(sa).all()) and bool(torch.isfinite(ea).all())
    assert torch.allclose(sa[:, 1:], sb[:, 1:], rtol=1e-9, atol=0) and torch.allclose(ea, eb, rtol=1e-9, atol=0), (B, M, N)
    assert float((sa[:, 0] - sb[:, 0]).abs().max()) < 1e-9, (B, M, N)
    nbytes = 4 * B * M * N
    ma, mb, mc = (statistics.median(t[k]) * 1e-3 for k in "abc")
    r = dict(shape=f"{B} x ({M} x {N})", B=B, M=M, N=N, R=2, trace_scores=stat(t["a"]), torch_fp64=stat(t["b"]), partial_stacks=stat(t["c"]),
             alg_bytes=nbytes, trace_scores_TBps=round(nbytes / ma / 1e12, 3), partial_stacks_TBps=round(nbytes / mc / 1e12, 3),
             fraction_of_partial_stacks_rate=round(mc / ma, 3), hbm_peak_fraction=round(nbytes / ma / HBM_PEAK, 3),
             torch_over_trace_scores=round(mb / ma, 1), sim_max_abs_diff=float(f"{float((sa[:, 0] - sb[:, 0]).abs().max()):.2e}"),
             stats=pl.trace_scores_stats(), stream_launches=int(pl.lib.tspws_hip_stream_launches(pl.h)))
    lines.append(r)
    print(json.dumps(r), flush=True)
    del pl, X, refs, P, out, sa, ea, sb, eb
    torch.cuda.empty_cache()

print(json.dumps(dict(tool="trace_scores_bench", warm=WARM, reps=REPS, device=torch.cuda.get_device_name(0),
                      headline_fraction_of_partial_stacks_rate=lines[0]["fraction_of_partial_stacks_rate"],
                      headline_torch_over_trace_scores=lines[0]["torch_over_trace_scores"])))
