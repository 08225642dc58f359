"""The convergence curves of many ensembles in one call (tspws_hip_convergence_batch, Plan.convergence_batch) on the GPU: every ensemble's
curves and step arrays against the oracle's tspws_main on that ensemble alone with an explicit reference trace (tests/conv_batch_ref.py),
against Plan.convergence on it, with the call's default references, with a small scratch budget in a child process.  The bounds are those of
test_convergence_vs_oracle (tests/test_hip_parity.py), per ensemble: similarities 1e-9 absolute, misfits 1e-7 max|expected| + 1e-18, step
arrays 2e-6 relative per row.  Curves and step arrays hold NaN before every call and the padding columns of the traces 1e30: an entry nobody
wrote, or a padding sample read into a sum, shows.

Shapes: N = 2048 with ld = N + 64 and first[0] = 3, ensembles of [1, 7, 0, 13, 70, 5] traces -- 70 crosses a 64-trace forward batch; with
Kmax = 6 the sizes 1 and 5 are all-incremental, 7 has exactly one two-stage step, 13 and 70 have groups of unequal size -- and N = 1501 (the
odd-length seam) with [9, 4] and Kmax = 3."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_batch_ref as cb

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))

SIZES, N, FIRST0, PAD, SEED = [1, 7, 0, 13, 70, 5], 2048, 3, 64, 11
# name -> (params, ensemble sizes, N)
CASES = {
    "default": (dict(), SIZES, N),
    "kmax6_unbiased": (dict(Kmax=6, unbiased=1), SIZES, N),
    "mexhat_wu1": (dict(type=-3, wu=1.0), SIZES, N),
    "kmax6_wu1.5": (dict(Kmax=6, wu=1.5), SIZES, N),
    "odd_seam": (dict(Kmax=3), [9, 4], 1501),
}


@pytest.fixture(scope="module")
def lib():
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    return lib


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def check_stats(st, kw, sizes):
    K = kw.get("Kmax", 0)
    two = sum(max(0, m - K) for m in sizes) if K else 0
    assert st["single_steps"] + st["two_stage_steps"] == sum(sizes), st
    assert st["two_stage_steps"] == two and st["rows"] == K * two, st
    assert st["empty"] == sum(1 for m in sizes if not m) and st["looped"] == 0 and st["rounds"] >= 1, st


@pytest.mark.parametrize("name", sorted(CASES))
def test_vs_oracle(lib, torch, name):
    kw, sizes, n = CASES[name]
    want = cb.expected(kw, sizes, n, FIRST0, SEED)
    r = cb.run(torch, kw, sizes, n, FIRST0, PAD, SEED)
    cb.check_written(r, sizes)
    check_stats(r["stats"], kw, sizes)
    if name.startswith("kmax6"):
        assert r["stats"]["two_stage_steps"] == 1 + 7 + 64 and r["stats"]["rows"] == 6 * 72, r["stats"]
    for b, m in enumerate(sizes):
        if m:
            cb.compare(cb.ensemble(r, r["first"], b), want[b], tag=f"{name} ensemble {b}")


@pytest.mark.parametrize("name", ["default", "kmax6_unbiased"])
def test_vs_single_call(lib, torch, name):
    """Plan.convergence on every ensemble alone, with its reference rows, gives the same curves to the bounds; a batch with ONE non-empty
    ensemble is that call bit for bit."""
    kw, sizes, n = CASES[name]
    r = cb.run(torch, kw, sizes, n, FIRST0, PAD, SEED)
    pl, f = r["plan"], r["first"]
    keys = ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps")
    single = {}
    for b, m in enumerate(sizes):
        if not m:
            continue
        out = pl.convergence(r["traces"][f[b]:f[b + 1]], r["R"][b], r["R"][b], steps=True)
        torch.cuda.synchronize()
        single[b] = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in zip(keys, out)}
        cb.compare(cb.ensemble(r, f, b), single[b], tag=f"{name} single call, ensemble {b}")
    # one non-empty ensemble (13 traces) between two empty ones
    b = 3
    f1 = np.array([f[b], f[b], f[b + 1], f[b + 1]], dtype=np.int64)
    R1 = r["R"][b].repeat(3, 1).contiguous()
    out = pl.convergence_batch(r["traces"], f1, R1, R1, steps=True)
    torch.cuda.synchronize()
    st = pl.convergence_batch_stats()
    assert st["looped"] == 1 and st["empty"] == 2 and st["single_steps"] + st["two_stage_steps"] == sizes[b], st
    for k, v in zip(keys, out):
        np.testing.assert_array_equal(v if isinstance(v, np.ndarray) else v.cpu().numpy(), single[b][k], err_msg=k)


def test_default_references(lib, torch):
    """Without references every ensemble is measured against its own final stacks (the rows of stack_batch, what tspws_main does without
    in->reference): the curves of Plan.convergence fed those rows, and the last ts-PWS step is the full stack -- similarity with its own
    float-rounded copy ~ 1."""
    kw, sizes, n = CASES["kmax6_unbiased"]
    r = cb.run(torch, kw, sizes, n, FIRST0, PAD, SEED, refs=None)
    cb.check_written(r, sizes)
    pl, f = r["plan"], r["first"]
    ls, ts = pl.stack_batch(r["traces"], f)
    keys = ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps")
    for b, m in enumerate(sizes):
        if not m:
            continue
        out = pl.convergence(r["traces"][f[b]:f[b + 1]], ts[b], ls[b], steps=True)
        torch.cuda.synchronize()
        want = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in zip(keys, out)}
        got = cb.ensemble(r, f, b)
        cb.compare(got, want, tag=f"default references, ensemble {b}")
        print("ensemble", b, "last ts-PWS similarity", got["conv_tsPWS_sim"][-1])
        assert abs(got["conv_tsPWS_sim"][-1] - 1.0) < 1e-6, (b, got["conv_tsPWS_sim"][-1])


@pytest.mark.parametrize("name", ["default", "kmax6_unbiased"])
def test_small_budget(lib, torch, tmp_path, name):
    """TSPWS_PART_MB = 16 (read once per process: a child): the steps take several rounds -- without a two-stage rule the 96 incremental
    steps are cut inside an ensemble and the running pair is carried, with Kmax = 6 the 72 two-stage steps take several rounds -- and the
    curves are those of the oracle to the bounds."""
    kw, sizes, n = CASES[name]
    want = cb.expected(kw, sizes, n, FIRST0, SEED)
    env = dict(os.environ, TSPWS_PART_MB="16")
    path = str(tmp_path / "small.npz")
    arg = json.dumps(dict(kw=kw, sizes=sizes, N=n, first0=FIRST0, pad=PAD, seed=SEED))
    out = subprocess.run([sys.executable, os.path.join(HERE, "conv_batch_ref.py"), arg, path], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "CONV_BATCH_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    r = dict(np.load(path))
    st = dict(zip(("single_steps", "two_stage_steps", "rows", "rounds", "looped", "empty"), r["stats"].tolist()))
    print(st)
    check_stats(st, kw, sizes)
    assert st["rounds"] > (2 if "Kmax" in kw else 1), st  # (more than the one round of each kind of the default budget)
    cb.check_written(r, sizes)
    f = cb.offsets(sizes, FIRST0)
    for b, m in enumerate(sizes):
        if m:
            cb.compare(cb.ensemble(r, f, b), want[b], tag=f"small budget, ensemble {b}")
