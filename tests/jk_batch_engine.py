"""Helpers of tests/test_jackknife_batch_gpu.py and its child process: the batched single-stage jackknife (Plan.jackknife_batch) under
per-process environment pins that the library reads once (TSPWS_ENGINE, TSPWS_PART_MB).  As a program, argv[1] = what to run:
  fir | spectral  the engine pin the parent set.  Cases whose total trace count reaches the many-trace rule under that engine must go through
                  the shared pass (Plan.jackknife_batch_stats), the others through one single call per ensemble; the spectral set of the
                  total is what the pin says (tspws_hip_spectral_choice); every ensemble's replicas against the trace-order restatement
                  (jk_single_ref.Restatement) and Plan.jackknife_single, its main rows against the oracle and Plan.stack_single
  budget          one batch of 44 classes of 130 traces (132 blocks: class 21 straddles the first two batches of the many-trace pass) against the
                  per-ensemble calls; twice in the process (bit-identical); under TSPWS_PART_MB=16 it must take several rounds (a class's plane
                  pair is 0.5 MB at N = 4096: at most 32 classes per round); the rows are
                  written to argv[2] (.npz) so that the parent compares the small-budget run with the default one
Prints JKB_CASE <name> <relerr> <stats> per case and JKB_DONE <worst> at the end; exits 1 on a case over 2e-6."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import jk_single_ref as ref

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")


def ensemble_times(sizes, seed):
    """Start times of every ensemble (leap_times: the never-deleted bin n occurs), concatenated; a single trace gets 31 December 2016."""
    out = []
    for b, m in enumerate(sizes):
        if m == 1:
            out.append(ref.leap_times(2, seed=seed)[-1:])
        elif m:
            out.append(ref.leap_times(m, seed=seed + b))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def run(torch, kw, sizes, N, nd=None, seed=1, first0=2, pad=5, sel=None, times=None, main=True):
    """One batched call on a padded device array (ld = N + pad) whose outputs held NaN (counts: 99) before it.  The selection comes from
    start times (nd = (n, d); `times` replaces ensemble_times) or is given.  Returns a dict of everything the checks need."""
    p = tspws.resolve(abi.default_params(**kw), N)
    pl = tspws.Plan(p, N)
    first = np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    if sel is None:
        t = np.concatenate([np.ones(first0, np.int64), ensemble_times(sizes, seed) if times is None else times])
        sel = tspws.jackknife_selection_batch(t, first, *nd)
    B, Cn = len(sizes), sel.shape[0]
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    nan = float("nan")
    ls = torch.full((B, N), nan, dtype=torch.float32, device="cuda") if main else None
    ts = torch.full((B, N), nan, dtype=torch.float32, device="cuda") if main else None
    jl = torch.full((B, Cn, N), nan, dtype=torch.float32, device="cuda")
    jt = torch.full((B, Cn, N), nan, dtype=torch.float32, device="cuda")
    jm = np.full((B, Cn), 99, np.uint32)
    out = pl.jackknife_batch(buf[:, :N], first, sel, ls, ts, jl, jt, jm, main=main)
    torch.cuda.synchronize()
    assert (out[0] is None and out[1] is None) if not main else (out[0] is ls and out[1] is ts)
    return dict(pl=pl, p=p, kw=kw, X=X, buf=buf, first=first, sel=sel, main=main, N=N, ls=ls.cpu().numpy() if main else None,
                ts=ts.cpu().numpy() if main else None, jl=jl.cpu().numpy(), jt=jt.cpu().numpy(), jm=jm, stats=pl.jackknife_batch_stats())


def check(torch, r, restatement=True, single=True):
    """Worst relerr of every row of every ensemble (asserting the exact parts): replicas with K_c > 0 against the trace-order restatement and
    Plan.jackknife_single on the ensemble alone, the main rows against the oracle's tspws_main and Plan.stack_single; replicas with K_c = 0 and
    empty ensembles must be exactly zero with count 0.  Nothing is skipped: an unwritten row is NaN and fails."""
    worst = 0.0
    first, f0, X, sel, pl = r["first"], int(r["first"][0]), r["X"], r["sel"], r["pl"]
    for k in ("jl", "jt") + (("ls", "ts") if r["main"] else ()):
        assert np.isfinite(r[k]).all(), f"{k}: rows the call did not write (NaN)"  # (max() below would let a NaN pass)
    for b in range(len(first) - 1):
        seg = np.ascontiguousarray(X[first[b]:first[b + 1]])
        sb = np.ascontiguousarray(sel[:, first[b] - f0:first[b + 1] - f0])
        jl, jt, jm = r["jl"][b], r["jt"][b], r["jm"][b]
        if not len(seg):
            assert not jm.any() and not (jl != 0).any() and not (jt != 0).any(), b
            if r["main"]:
                assert not (r["ls"][b] != 0).any() and not (r["ts"][b] != 0).any(), b
            continue
        np.testing.assert_array_equal(jm, (sb == 1).sum(axis=1))
        wants = []
        if restatement:
            wants.append(ref.Restatement(r["p"], seg).replicas(sb))
        if single:
            segd = torch.from_numpy(seg).cuda()
            a, c, m = pl.jackknife_single(segd, sb)
            torch.cuda.synchronize()
            wants.append((a.cpu().numpy(), c.cpu().numpy(), m))
        for wl, wt, wm in wants:
            np.testing.assert_array_equal(jm, wm)
            for c in range(len(wm)):
                if wm[c]:
                    assert np.abs(wt[c]).max() > 0 and np.abs(wl[c]).max() > 0, (b, c)  # (the comparison is not between two zero rows)
                    worst = max(worst, abi.relerr(jt[c], wt[c]), abi.relerr(jl[c], wl[c]))
                else:
                    assert not (jt[c] != 0).any() and not (jl[c] != 0).any(), (b, c)
        if r["main"]:
            if restatement:
                w = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(**r["kw"]), seg)
                assert w["rc"] == 0
                worst = max(worst, abi.relerr(r["ls"][b], w["ls"]), abi.relerr(r["ts"][b], w["tsPWS"]))
            if single:
                l1, t1 = pl.stack_single(torch.from_numpy(seg).cuda())
                torch.cuda.synchronize()
                worst = max(worst, abi.relerr(r["ls"][b], l1.cpu().numpy()), abi.relerr(r["ts"][b], t1.cpu().numpy()))
    assert np.isfinite(worst)
    return worst


def budget_batch(torch):
    """22 ensembles of 260 traces, two classes of 130 (three blocks) each: 132 blocks, so class 21 (blocks 63-65) straddles the first two batches
    of the many-trace pass (64 blocks each).  Replicas: first half only, second half only, everything, nothing."""
    sizes = [260] * 22
    one = np.zeros((4, 260), np.int8)
    one[0, :130] = 1
    one[1, 130:] = 1
    one[2, :] = 1
    return run(torch, dict(unbiased=1), sizes, 4096, seed=5, first0=1, pad=0, sel=np.ascontiguousarray(np.tile(one, (1, 22))))


if __name__ == "__main__":
    import torch

    lib = tspws.load()
    mode = sys.argv[1]
    worst, bad = 0.0, []

    def report(name, e, stats):
        global worst
        print("JKB_CASE", name, f"{e:.3e}", stats, flush=True)
        worst = max(worst, e)
        if not e < TOL32:
            bad.append(name)

    if mode in ("fir", "spectral"):
        assert os.environ.get("TSPWS_ENGINE") == mode
        # (name, params, sizes, N, (n, d), shared pass under fir, under spectral).  The FIR-only many-trace rule: > 2 voices per octave, >= 128
        # traces and >= 7 M samples (forward.hip); the spectral pin sends every batch of a frame with a spectral set there.
        CASES = [
            ("morlet_4096", dict(), [0, 1, 40, 64, 65, 130], 4096, (4, 1), False, True),                  # 1.2 M samples
            ("mexhat_1501_unbiased", dict(type=-2, unbiased=1), [30, 64, 65, 130], 1501, (5, 2), False, True),
            ("morlet_16501", dict(), [130, 65, 260], 16501, (12, 1), True, True),                        # 7.5 M samples: clipped scales too
        ]
        shared_fir = 0
        for name, kw, sizes, N, nd, on_fir, on_spec in CASES:
            r = run(torch, kw, sizes, N, nd, seed=11)
            pl, st = r["pl"], r["stats"]
            total = int(r["first"][-1] - r["first"][0])
            nonempty = sum(1 for m in sizes if m)
            choice = lib.tspws_hip_spectral_choice(pl.h, total)
            if mode == "fir":
                assert choice == pl.S, (name, choice)  # no spectral set: the shared pass, where taken, runs the FIR-only many-trace kernels
            else:
                assert choice < pl.S, (name, choice)
            assert st["empty"] == len(sizes) - nonempty, (name, st)
            if on_fir if mode == "fir" else on_spec:
                assert st["shared"] == nonempty and st["looped"] == 0 and st["pass_batches"] >= 1, (name, st)
                shared_fir += mode == "fir"
            else:
                assert st["shared"] == 0 and st["looped"] == nonempty, (name, st)
            report(name, check(torch, r), st)
        assert mode != "fir" or shared_fir == 1
    elif mode == "budget":
        small = "TSPWS_PART_MB" in os.environ
        r = budget_batch(torch)
        st = r["stats"]
        assert st["shared"] == 22 and st["looped"] == 0 and st["classes"] == 44 and st["pass_batches"] >= 2, st
        assert (st["rounds"] > 1) if small else (st["rounds"] == 1), st
        report("budget", check(torch, r, restatement=False), st)
        r2 = budget_batch(torch)  # the same call again in this process: bit-identical
        for k in ("ls", "ts", "jl", "jt", "jm"):
            assert np.array_equal(r[k], r2[k]), k
        np.savez(sys.argv[2], ls=r["ls"], ts=r["ts"], jl=r["jl"], jt=r["jt"], jm=r["jm"])
    else:
        raise SystemExit(f"unknown mode {mode}")

    print("JKB_DONE", f"{worst:.3e}", flush=True)
    sys.exit(1 if bad else 0)
