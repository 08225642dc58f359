"""Helpers of tests/test_subsample_batch_gpu.py and its child processes: the batched random subsampling (Plan.subsample_batch).  Outputs hold
NaN (counts: 99) before every call.  Masks drawn from a probability are drawn ensemble by ensemble, each after abi.srand(seeds[b]), and every
ensemble's block is compared with
  (i)  the oracle's tspws_main on the ensemble alone with subsmpl_N = M, after the same abi.srand(seeds[b]) (it draws the same masks), and
  (ii) Plan.subsample_sel on the ensemble alone with its columns;
arbitrary masks are compared with (ii) one row at a time, with subsmpl_p chosen so that ceil(M_b p) == K.  Rows that keep nothing and empty
ensembles must be exactly zero with count 0; no compared reference row may be all zero.  Nothing is skipped: an unwritten row is NaN and fails.
As a program, argv[1] = "budget", argv[2] = an .npz path: 12 single-stage ensembles of 40 x 4096, M = 8, p = 0.5 under the TSPWS_PART_MB of
the environment (the library reads it once per process) against reference (ii), twice in the process (bit-identical); with a budget set the
call must take several rounds (the partials of the 480 traces and the 96 plane pairs are far beyond 16 MB), without one it takes one; the
rows are written to argv[2] so that the parent compares the two runs.  Prints SUB_CASE / SUB_DONE <worst>; exits 1 on a case over 2e-6."""
import importlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")


def offsets(sizes, first0):
    return np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)


def draw(sizes, M, prob, seeds):
    """Masks [M][T]: ensemble b's columns drawn by the library's host function right after abi.srand(seeds[b])."""
    sel = np.zeros((M, int(sum(sizes))), np.int8)
    c0 = 0
    for b, mb in enumerate(sizes):
        abi.srand(seeds[b])
        sel[:, c0:c0 + mb] = tspws.subsampling_selection_batch([0, mb], M, prob)
        c0 += mb
    return sel


def run(torch, kw, sizes, N, sel, prob=0.5, seed=1, first0=2, pad=5):
    """One batched call on a padded device array (ld = N + pad) whose outputs held NaN (counts: 99) before it."""
    M = sel.shape[0]
    p = tspws.resolve(abi.default_params(subsmpl_N=M, subsmpl_p=prob, **kw), N)
    pl = tspws.Plan(p, N)
    first = offsets(sizes, first0)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    r = dict(pl=pl, p=p, kw=kw, X=X, buf=buf, first=first, sel=sel, prob=prob, N=N, M=M, sizes=list(sizes))
    call(torch, r)
    return r


def call(torch, r):
    """The batched call of `r` again on NaN-filled outputs."""
    B, M, N = len(r["sizes"]), r["M"], r["N"]
    nan = float("nan")
    sl = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    st = torch.full((B, M, N), nan, dtype=torch.float32, device="cuda")
    sm = np.full((B, M), 99, np.uint32)
    out = r["pl"].subsample_batch(r["buf"][:, :N], r["first"], r["sel"], sl, st, sm)
    torch.cuda.synchronize()
    assert out[0] is sl and out[1] is st and out[2] is sm
    r.update(sl=sl.cpu().numpy(), st=st.cpu().numpy(), sm=sm, stats=r["pl"].subsample_batch_stats())
    return r


def blocks(r):
    """(b, traces of ensemble b, its mask columns) for every ensemble, after the checks every case shares."""
    for k in ("sl", "st"):
        assert np.isfinite(r[k]).all(), f"{k}: rows the call did not write (NaN)"  # (max() would let a NaN pass)
    first, f0 = r["first"], int(r["first"][0])
    for b in range(len(first) - 1):
        seg = np.ascontiguousarray(r["X"][first[b]:first[b + 1]])
        sb = np.ascontiguousarray(r["sel"][:, first[b] - f0:first[b + 1] - f0])
        np.testing.assert_array_equal(r["sm"][b], (sb == 1).sum(axis=1))
        if not len(seg):
            assert not r["sm"][b].any() and not (r["sl"][b] != 0).any() and not (r["st"][b] != 0).any(), b
            continue
        yield b, seg, sb


def check(torch, r, seeds, oracle=True, single=True):
    """Masks from a probability: worst relerr of every block against references (i) and (ii); counts equal ceil(M_b p)."""
    worst = 0.0
    assert oracle or single
    for b, seg, sb in blocks(r):
        K = math.ceil(len(seg) * r["prob"])
        assert K > 0 and (r["sm"][b] == K).all(), (b, K, r["sm"][b])
        wants = []
        if oracle:
            abi.srand(seeds[b])
            w = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(subsmpl_N=r["M"], subsmpl_p=r["prob"], **r["kw"]), seg)
            assert w["rc"] == 0
            wants.append((w["sub_ls"], w["sub_ts"]))
        if single:
            l1, t1 = r["pl"].subsample_sel(torch.from_numpy(seg).cuda(), sb)
            torch.cuda.synchronize()
            wants.append((l1.cpu().numpy(), t1.cpu().numpy()))
        for wl, wt in wants:
            for m in range(r["M"]):
                assert np.abs(wl[m]).max() > 0 and np.abs(wt[m]).max() > 0, (b, m)  # (the comparison is not between two zero rows)
                el, et = abi.relerr(r["sl"][b, m], wl[m]), abi.relerr(r["st"][b, m], wt[m])
                assert np.isfinite(el) and np.isfinite(et), (b, m)
                worst = max(worst, el, et)
    return worst


def check_rows(torch, r):
    """Arbitrary masks: every row with K > 0 against Plan.subsample_sel on that row alone with ceil(M_b p) == K; K = 0: exact zeros."""
    worst, n = 0.0, 0
    for b, seg, sb in blocks(r):
        Xd = torch.from_numpy(seg).cuda()
        for m in range(r["M"]):
            K = int(r["sm"][b, m])
            if not K:
                assert not (r["sl"][b, m] != 0).any() and not (r["st"][b, m] != 0).any(), (b, m)
                continue
            prob = (K - 0.5) / len(seg)
            assert math.ceil(len(seg) * prob) == K
            l1, t1 = r["pl"].subsample_sel(Xd, np.ascontiguousarray(sb[m:m + 1]), prob=prob)
            torch.cuda.synchronize()
            wl, wt = l1.cpu().numpy()[0], t1.cpu().numpy()[0]
            assert np.abs(wl).max() > 0 and np.abs(wt).max() > 0, (b, m)
            el, et = abi.relerr(r["sl"][b, m], wl), abi.relerr(r["st"][b, m], wt)
            assert np.isfinite(el) and np.isfinite(et), (b, m)
            worst = max(worst, el, et)
            n += 1
    assert n
    return worst


BUDGET_SIZES, BUDGET_M, BUDGET_P = [40] * 12, 8, 0.5


def budget_batch(torch):
    seeds = [100 + b for b in range(len(BUDGET_SIZES))]
    return run(torch, dict(), BUDGET_SIZES, 4096, draw(BUDGET_SIZES, BUDGET_M, BUDGET_P, seeds), prob=BUDGET_P, seed=5, first0=1, pad=0), seeds


if __name__ == "__main__":
    import torch

    mode = sys.argv[1]
    if mode != "budget":
        raise SystemExit(f"unknown mode {mode}")
    small = "TSPWS_PART_MB" in os.environ
    r, seeds = budget_batch(torch)
    st = r["stats"]
    assert st["single_shared"] == 12 and st["two_stage_shared"] == 0 and st["looped"] == 0 and st["empty"] == 0 and st["rows"] == 12 * BUDGET_M, st
    assert (st["rounds"] > 1) if small else (st["rounds"] == 1), st
    first = {k: r[k].copy() for k in ("sl", "st", "sm")}
    e = check(torch, r, seeds, oracle=False)
    print("SUB_CASE", "budget", f"{e:.3e}", st, flush=True)
    call(torch, r)  # the same call again in this process: bit-identical
    for k in ("sl", "st", "sm"):
        assert np.array_equal(first[k], r[k]), k
    np.savez(sys.argv[2], sl=r["sl"], st=r["st"], sm=r["sm"])
    print("SUB_DONE", f"{e:.3e}", flush=True)
    sys.exit(0 if e < TOL32 else 1)
