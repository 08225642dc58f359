"""Child process of tests/test_stack_batch_gpu.py: batched stacks (Plan.stack_batch) under per-process environment pins that the library
reads once (TSPWS_ENGINE, TSPWS_PART_MB).  argv[1] = what to run:
  fir | spectral  the engine pin the parent set.  Cases whose total trace count reaches the many-trace rule under that engine must go through
                  the shared pass (Plan.batch_stats), the others through one single call per ensemble; the spectral set of the total is what
                  the pin says (tspws_hip_spectral_choice: none under fir, so the shared pass runs the FIR-only many-trace kernels); every
                  ensemble within 2e-6 of the oracle and of Plan.stack_single on that ensemble alone
  chunks          a single-stage batch whose ensembles straddle the batches of the many-trace pass, and a two-stage batch; every ensemble
                  against Plan.stack_single; under TSPWS_PART_MB the two-stage batch must take several rounds (one with the default budget);
                  the rows are written to argv[2] (.npz) so that the parent compares a small-budget run with a default one
Prints BATCH_CASE <name> <relerr> <stats> per case and BATCH_DONE <worst> at the end; exits 1 on a case over 2e-6."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import torch

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")
lib = tspws.load()
mode = sys.argv[1]
worst, bad = 0.0, []


def batch(kw, sizes, N, seed, first0=2, pad=5):
    """(plan, params, traces [mtr][N] numpy, offsets, ls, ts, stats) of one batched call on a padded device array (ld = N + pad)."""
    p = abi.default_params(**kw)
    pl = tspws.Plan(tspws.resolve(p, N), N)
    first = np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    ls, ts = pl.stack_batch(buf[:, :N], first)
    torch.cuda.synchronize()
    return pl, p, X, first, ls.cpu().numpy(), ts.cpu().numpy(), pl.batch_stats()


def check(name, pl, p, X, first, ls, ts, stats, oracle=True):
    global worst
    e = 0.0
    for b in range(len(first) - 1):
        seg = X[first[b]:first[b + 1]]
        if not len(seg):
            assert not ls[b].any() and not ts[b].any(), (name, b)
            continue
        l1, t1 = pl.stack_single(torch.from_numpy(np.ascontiguousarray(seg)).cuda())
        torch.cuda.synchronize()
        e = max(e, abi.relerr(ls[b], l1.cpu().numpy()), abi.relerr(ts[b], t1.cpu().numpy()))
        if oracle:
            w = abi.run_main(abi.oracle().orc_tspws_main, p, seg)
            assert w["rc"] == 0
            e = max(e, abi.relerr(ls[b], w["ls"]), abi.relerr(ts[b], w["tsPWS"]))
    print("BATCH_CASE", name, f"{e:.3e}", stats, flush=True)
    worst = max(worst, e)
    if not e < TOL32:
        bad.append(name)


if mode in ("fir", "spectral"):
    assert os.environ.get("TSPWS_ENGINE") == mode
    # (name, params, sizes, N, shared pass under fir, under spectral).  The FIR-only many-trace rule: > 2 voices per octave, >= 128 traces and
    # >= 7 M samples (forward.hip); the spectral pin sends every batch of a frame with a spectral set there.
    CASES = [
        ("morlet_4096", dict(), [0, 1, 63, 64, 65, 130, 499], 4096, False, True),         # 3.4 M samples
        ("mexhat_1501_unbiased", dict(type=-2, unbiased=1), [30, 64, 65, 130], 1501, False, True),  # two voices
        ("type3_16501_wu", dict(type=-3, wu=1.3), [1, 64, 130, 65], 16501, False, True),  # 4.3 M samples
        ("morlet_16501", dict(), [0, 1, 63, 64, 65, 130, 499], 16501, True, True),       # 13.6 M samples: clipped scales too
        ("morlet_4096_61x30_unbiased", dict(unbiased=1), [30] * 61, 4096, True, True),   # 7.5 M samples in 61 small ensembles
    ]
    shared_fir = 0
    for name, kw, sizes, N, on_fir, on_spec in CASES:
        pl, p, X, first, ls, ts, st = batch(kw, sizes, N, seed=11)
        total = int(first[-1] - first[0])
        nonempty = sum(1 for m in sizes if m)
        choice = lib.tspws_hip_spectral_choice(pl.h, total)
        if mode == "fir":
            assert choice == pl.S, (name, choice)  # no spectral set: the shared pass, where taken, runs the FIR-only many-trace kernels
        else:
            assert choice < pl.S, (name, choice)
        shared = on_fir if mode == "fir" else on_spec
        assert st["empty"] == len(sizes) - nonempty and st["two_stage_pass"] == 0, (name, st)
        if shared:
            assert st["single_pass"] == nonempty and st["looped"] == 0 and st["pass_batches"] >= 1, (name, st)
            shared_fir += mode == "fir"
        else:
            assert st["single_pass"] == 0 and st["looped"] == nonempty, (name, st)
        check(name, pl, p, X, first, ls, ts, st)
    assert mode != "fir" or shared_fir == 2
elif mode == "chunks":
    small = "TSPWS_PART_MB" in os.environ
    # 40 ensembles of 3 blocks (130 traces) = 120 blocks: more than the 64 blocks of one batch of the pass, so ensemble 21 (blocks 63-65)
    # straddles two batches
    pl, p, X, first, ls1, ts1, st = batch(dict(), [130] * 40, 4096, seed=5, first0=1, pad=0)
    assert st["single_pass"] == 40 and st["pass_batches"] >= 2, st
    check("single_straddle", pl, p, X, first, ls1, ts1, st, oracle=False)
    # two-stage, Kmax = 10: 24 ensembles of 10 .. 80 traces (and a single-stage one of 5, alone of its kind: one single call)
    sizes = [int(m) for m in np.random.default_rng(3).integers(10, 81, 24)] + [5]
    pl, p, X, first, ls2, ts2, st = batch(dict(Kmax=10, unbiased=1), sizes, 4096, seed=6)
    assert st["two_stage_pass"] == 24 and st["looped"] == 1, st
    assert (st["rounds"] > 1) if small else (st["rounds"] == 1), st
    check("two_stage_rounds", pl, p, X, first, ls2, ts2, st, oracle=False)
    np.savez(sys.argv[2], ls1=ls1, ts1=ts1, ls2=ls2, ts2=ts2)
else:
    raise SystemExit(f"unknown mode {mode}")

print("BATCH_DONE", f"{worst:.3e}", flush=True)
sys.exit(1 if bad else 0)
