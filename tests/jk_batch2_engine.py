"""Helpers of tests/test_jackknife_batch_two_stage_gpu.py and its child process: the batched two-stage jackknife
(Plan.jackknife_batch_two_stage).  Outputs hold NaN (counts: 99) before every call; every row with K_c > 0 is compared with
  (i)  the oracle's tspws_main on the ensemble alone with its start times (ls, tsPWS, the jackknife rows and counts) -- selections that come
       from start times only --, and
  (ii) Plan.stack_jackknife on the ensemble alone;
every row with K_c = 0 and every empty ensemble must be exactly zero with count 0.  Nothing is skipped: an unwritten row is NaN and fails.
As a program, argv[1] = "budget", argv[2] = an .npz path: 12 ensembles of 40 x 4096 (Kmax = 10, n = 12, d = 1) under the TSPWS_PART_MB of the
environment (the library reads it once per process) against reference (ii), twice in the process (bit-identical); with a budget set the call
must take several rounds (an ensemble's 13 x 10 rows are 4.3 MB), without one it takes one; the rows are written to argv[2] so that the parent
compares the two runs.  Prints JK2_CASE <name> <relerr> <stats> and JK2_DONE <worst>; exits 1 on a case over 2e-6."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
from jk_batch_engine import ensemble_times

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")


def run(torch, kw, sizes, N, nd=None, seed=1, first0=2, pad=5, sel=None, times=None, main=True):
    """One batched call on a padded device array (ld = N + pad) whose outputs held NaN (counts: 99) before it.  The selection comes from
    start times (nd = (n, d); `times` replaces ensemble_times) or is given.  Returns a dict of everything the checks need."""
    p = tspws.resolve(abi.default_params(**kw), N)
    pl = tspws.Plan(p, N)
    first = np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    if sel is None:
        times = ensemble_times(sizes, seed) if times is None else times
        sel = tspws.jackknife_selection_batch(np.concatenate([np.ones(first0, np.int64), times]), first, *nd)
    else:
        nd = times = None
    B, Cn = len(sizes), sel.shape[0]
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    nan = float("nan")
    ls = torch.full((B, N), nan, dtype=torch.float32, device="cuda") if main else None
    ts = torch.full((B, N), nan, dtype=torch.float32, device="cuda") if main else None
    jl = torch.full((B, Cn, N), nan, dtype=torch.float32, device="cuda")
    jt = torch.full((B, Cn, N), nan, dtype=torch.float32, device="cuda")
    jm = np.full((B, Cn), 99, np.uint32)
    out = pl.jackknife_batch_two_stage(buf[:, :N], first, sel, ls, ts, jl, jt, jm, main=main)
    torch.cuda.synchronize()
    assert (out[0] is None and out[1] is None) if not main else (out[0] is ls and out[1] is ts)
    assert out[2] is jl and out[3] is jt and out[4] is jm
    return dict(pl=pl, p=p, kw=kw, X=X, buf=buf, first=first, sel=sel, nd=nd, times=times, main=main, N=N, ls=ls.cpu().numpy() if main else None,
                ts=ts.cpu().numpy() if main else None, jl=jl.cpu().numpy(), jt=jt.cpu().numpy(), jm=jm, stats=pl.jackknife_batch_two_stage_stats())


def check(torch, r, oracle=True, single=True):
    """Worst relerr of every row of every ensemble against references (i) and (ii), asserting the exact parts."""
    worst = 0.0
    first, f0, X, sel, pl = r["first"], int(r["first"][0]), r["X"], r["sel"], r["pl"]
    oracle = oracle and r["nd"] is not None
    assert oracle or single
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
        wants = []  # (ls, ts, jk_ls, jk_ts, jk_mtr)
        if oracle:
            n, d = r["nd"]
            w = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(jackknife_n=n, jackknife_d=d, **r["kw"]), seg,
                             times=r["times"][first[b] - f0:first[b + 1] - f0])
            assert w["rc"] == 0
            wants.append((w["ls"], w["tsPWS"], w["jk_ls"], w["jk_ts"], w["jk_mtr"]))
        if single:
            l1, t1, a, c, m = pl.stack_jackknife(torch.from_numpy(seg).cuda(), sb)
            torch.cuda.synchronize()
            wants.append((l1.cpu().numpy(), t1.cpu().numpy(), a.cpu().numpy(), c.cpu().numpy(), m))
        for wls, wts, wl, wt, wm in wants:
            np.testing.assert_array_equal(jm, wm)
            for c in range(len(wm)):
                if wm[c]:
                    assert np.abs(wt[c]).max() > 0 and np.abs(wl[c]).max() > 0, (b, c)  # (the comparison is not between two zero rows)
                    worst = max(worst, abi.relerr(jt[c], wt[c]), abi.relerr(jl[c], wl[c]))
                else:
                    assert not (jt[c] != 0).any() and not (jl[c] != 0).any(), (b, c)
            if r["main"]:
                assert np.abs(wls).max() > 0 and np.abs(wts).max() > 0, b
                worst = max(worst, abi.relerr(r["ls"][b], wls), abi.relerr(r["ts"][b], wts))
    assert np.isfinite(worst)
    return worst


def budget_batch(torch):
    return run(torch, dict(unbiased=1, Kmax=10), [40] * 12, 4096, (12, 1), seed=5, first0=1, pad=0)


if __name__ == "__main__":
    import torch

    mode = sys.argv[1]
    if mode != "budget":
        raise SystemExit(f"unknown mode {mode}")
    small = "TSPWS_PART_MB" in os.environ
    r = budget_batch(torch)
    st = r["stats"]
    assert st["shared"] == 12 and st["looped"] == 0 and st["empty"] == 0 and st["tiles"] == 1 and st["rows"] == 12 * 13 * 10, st
    assert (st["rounds"] > 1) if small else (st["rounds"] == 1), st
    e = check(torch, r, oracle=False)
    print("JK2_CASE", "budget", f"{e:.3e}", st, flush=True)
    r2 = budget_batch(torch)  # the same call again in this process: bit-identical
    for k in ("ls", "ts", "jl", "jt", "jm"):
        assert np.array_equal(r[k], r2[k]), k
    np.savez(sys.argv[2], ls=r["ls"], ts=r["ts"], jl=r["jl"], jt=r["jt"], jm=r["jm"])
    print("JK2_DONE", f"{e:.3e}", flush=True)
    sys.exit(0 if e < TOL32 else 1)
