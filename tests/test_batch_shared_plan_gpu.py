"""The batched entry points share three scratch slots of the plan (the round's tables, the weighted sets of a finish batch, their
reconstructions).  On ONE plan the five batched calls run in turn -- stack_batch, jackknife_batch, jackknife_batch_two_stage,
convergence_batch, subsample_batch with single- and two-stage ensembles mixed -- with only pl.params changed in between, then again in
reverse order on a larger batch, so that the shared slots regrow between units.  Every output must be bit-identical to the same call on a
fresh plan, and the stats calls must say that the shared paths ran (not the per-ensemble loops)."""
import importlib

import numpy as np
import pytest

import abi

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N, C, M = 4096, 9, 9
# (ensemble sizes; the last two are single-stage under Kmax = 10 and are left out of the two-stage jackknife)
BATCHES = ([40] * 10 + [6, 8], [70] * 12 + [7, 9])


def new_plan():
    return tspws.Plan(tspws.resolve(abi.default_params(), N), N)


def two_stage(pl, on):
    pl.params.Kmax, pl.params.unbiased = (10, 1) if on else (0, 0)


def bins_selection(sizes):
    """[C][T] delete-one selection: trace i of an ensemble sits in bin i % C, column c drops bin c."""
    sel = np.ones((C, sum(sizes)), np.int8)
    t = 0
    for m in sizes:
        sel[np.arange(m) % C, t + np.arange(m)] = 0
        t += m
    return sel


def the_calls(torch, sizes, seed):
    """name -> call(plan) -> list of numpy outputs; every call sets pl.params itself and asserts that its shared path ran."""
    B = len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = tspws.synth(int(first[-1]), N, seed=seed)
    sel = bins_selection(sizes)
    big = B - 2  # the ensembles that are two-stage under Kmax = 10
    tb = int(first[big])
    masks = (np.random.default_rng(seed).random((M, int(first[-1]))) < 0.6).astype(np.int8)
    ref_ls = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    ref_ts = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    ref_ls[:, 100:200] = 1.0
    ref_ts[:, 150:300] = -0.5

    def stack(pl):
        two_stage(pl, False)
        out = pl.stack_batch(X, first)
        st = pl.batch_stats()
        assert st["single_pass"] == B and st["looped"] == 0, st
        return out

    def jk(pl):
        two_stage(pl, False)
        out = pl.jackknife_batch(X, first, sel)
        st = pl.jackknife_batch_stats()
        assert st["shared"] == B and st["looped"] == 0 and st["rounds"] >= 1, st
        return out

    def jk2(pl):
        two_stage(pl, True)
        out = pl.jackknife_batch_two_stage(X, first[:big + 1], np.ascontiguousarray(sel[:, :tb]))
        st = pl.jackknife_batch_two_stage_stats()
        assert st["shared"] == big and st["looped"] == 0 and st["rounds"] >= 1, st
        return out

    def conv(pl):
        two_stage(pl, True)
        out = pl.convergence_batch(X, first, ref_ts, ref_ls, steps=True)
        st = pl.convergence_batch_stats()
        assert st["looped"] == 0 and st["single_steps"] > 0 and st["two_stage_steps"] > 0 and st["rounds"] >= 2, st
        return out

    def sub(pl):
        two_stage(pl, True)
        out = pl.subsample_batch(X, first, masks)
        st = pl.subsample_batch_stats()
        assert st["single_shared"] == 2 and st["two_stage_shared"] == big and st["looped"] == 0, st
        return out

    def host(fn):
        def run(pl):
            out = [a.cpu().numpy() if isinstance(a, torch.Tensor) else np.array(a) for a in fn(pl)]
            torch.cuda.synchronize()
            return out
        return run
    return [(f.__name__, host(f)) for f in (stack, jk, jk2, conv, sub)]


def test_one_plan_serves_every_batched_call():
    import torch
    assert torch.cuda.is_available()
    shared = new_plan()
    for k, sizes in enumerate(BATCHES):
        calls = the_calls(torch, sizes, seed=11 + k)
        for name, call in (calls if k == 0 else calls[::-1]):  # the larger batch in reverse order
            got = call(shared)
            fresh = new_plan()
            want = call(fresh)
            fresh.close()
            assert len(got) == len(want)
            for j, (g, w) in enumerate(zip(got, want)):
                assert g.size and np.isfinite(g).all(), (k, name, j)
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (k, name, j)
            assert any(np.abs(g).max() > 0 for g in got), (k, name)
    shared.close()
