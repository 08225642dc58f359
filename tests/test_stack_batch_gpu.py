"""Many same-length ensembles in one call (tspws_hip_stack_batch, Plan.stack_batch) on the GPU: every ensemble's row against the oracle
on that ensemble alone and against Plan.stack_single on it; engines pinned per process (tests/batch_engine.py), ensembles that straddle the
many-trace pass's batches and a small scratch budget, determinism, B = 1, argument errors."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi

pytestmark = pytest.mark.gpu

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))


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


def run_batch(torch, kw, sizes, N, seed, first0=3, pad=7):
    p = abi.default_params(**kw)
    pl = tspws.Plan(tspws.resolve(p, N), N)
    first = np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    ls, ts = pl.stack_batch(buf[:, :N], first)
    torch.cuda.synchronize()
    return pl, p, X, first, buf, ls.cpu().numpy(), ts.cpu().numpy()


def check_rows(torch, pl, p, X, first, ls, ts):
    for b in range(len(first) - 1):
        seg = X[first[b]:first[b + 1]]
        if not len(seg):
            assert not ls[b].any() and not ts[b].any(), b
            continue
        want = abi.run_main(abi.oracle().orc_tspws_main, p, seg)
        assert want["rc"] == 0
        assert abi.relerr(ts[b], want["tsPWS"]) < TOL32, (b, len(seg))
        assert abi.relerr(ls[b], want["ls"]) < TOL32, (b, len(seg))
        l1, t1 = pl.stack_single(torch.from_numpy(np.ascontiguousarray(seg)).cuda())
        torch.cuda.synchronize()
        assert abi.relerr(ts[b], t1.cpu().numpy()) < TOL32, (b, len(seg))
        assert abi.relerr(ls[b], l1.cpu().numpy()) < TOL32, (b, len(seg))


# (params, ensemble sizes, N): types -1 / -2 / -3, unbiased, wu = 1.3; N = 1501 / 16 501 take the any-N spectral path (16 501: with the
# contraction of the clipped scales); sizes 0, 1, 63, 64, 65, 130, 499 in one batch; a batch of one ensemble per size below the many-trace
# threshold (one tspws_hip_stack per ensemble)
CASES = [
    (dict(), [0, 1, 63, 64, 65, 130, 499], 4096),
    (dict(type=-2, unbiased=1), [65, 0, 130, 1, 64], 1501),
    (dict(type=-3, wu=1.3), [64, 1, 130, 65, 0], 16501),
    (dict(unbiased=1), [63, 1, 0], 4096),
]


@pytest.mark.parametrize("kw,sizes,N", CASES)
def test_batch_parity(lib, torch, kw, sizes, N):
    pl, p, X, first, _, ls, ts = run_batch(torch, kw, sizes, N, seed=sum(sizes) + N)
    st = pl.batch_stats()
    nonempty = sum(1 for m in sizes if m)
    if sum(sizes) >= 256:  # (the default engine takes the many-trace path for the total: the shared pass)
        assert lib.tspws_hip_spectral_choice(pl.h, sum(sizes)) < pl.S
        assert st["single_pass"] == nonempty and st["looped"] == 0, st
    else:
        assert st["single_pass"] == 0 and st["looped"] == nonempty, st
    check_rows(torch, pl, p, X, first, ls, ts)


def test_two_stage_mixed(lib, torch):
    # Kmax = 10: the ensemble of 5 is single-stage by the rule (Kmax > M), the others two-stage; a second single-stage ensemble of 3
    pl, p, X, first, _, ls, ts = run_batch(torch, dict(Kmax=10), [5, 10, 11, 300, 3, 0], 4096, seed=7)
    st = pl.batch_stats()
    assert st["two_stage_pass"] == 3 and st["looped"] == 2 and st["empty"] == 1, st
    check_rows(torch, pl, p, X, first, ls, ts)


def test_two_stage_unbiased_any_n(lib, torch):
    pl, p, X, first, _, ls, ts = run_batch(torch, dict(Kmax=10, unbiased=1, type=-2), [40, 12, 10, 64], 1501, seed=8)
    assert pl.batch_stats()["two_stage_pass"] == 4
    check_rows(torch, pl, p, X, first, ls, ts)


@pytest.mark.parametrize("engine", ["fir", "spectral"])
def test_engines(engine):
    env = dict(os.environ, TSPWS_ENGINE=engine)
    out = subprocess.run([sys.executable, os.path.join(HERE, "batch_engine.py"), engine], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "BATCH_DONE" in out.stdout


def test_chunks_small_budget(tmp_path):
    """A single-stage batch whose ensembles straddle the batches of the many-trace pass and a two-stage batch, with the default budget and with
    16 MB (the two-stage ensembles then take several rounds; a round never splits an ensemble): every row matches Plan.stack_single in the
    child, and the two runs match each other, to the tolerance."""
    res = {}
    for tag, extra in (("default", {}), ("small", {"TSPWS_PART_MB": "16"})):
        env = dict(os.environ)
        env.pop("TSPWS_PART_MB", None)
        env.update(extra)
        path = str(tmp_path / f"{tag}.npz")
        out = subprocess.run([sys.executable, os.path.join(HERE, "batch_engine.py"), "chunks", path], capture_output=True, text=True, env=env,
                             timeout=900)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        res[tag] = np.load(path)
    for k in ("ls1", "ts1", "ls2", "ts2"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            assert abi.relerr(b[r], a[r]) < TOL32, (k, r)


def test_deterministic_and_single(lib, torch):
    pl, p, X, first, buf, ls, ts = run_batch(torch, dict(), [70, 30, 130, 64], 4096, seed=3)
    ls2, ts2 = pl.stack_batch(buf[:, :4096], first)
    torch.cuda.synchronize()
    assert np.array_equal(ls, ls2.cpu().numpy()) and np.array_equal(ts, ts2.cpu().numpy())
    # B = 1 over a whole ensemble IS tspws_hip_stack: bit-identical (single- and two-stage)
    for kw in (dict(), dict(Kmax=10)):
        p1 = abi.default_params(**kw)
        pl1 = tspws.Plan(tspws.resolve(p1, 4096), 4096)
        seg = buf[3:3 + 130, :4096]
        l1, t1 = pl1.stack_batch(seg, [0, 130])
        l0, t0 = pl1.stack_single(seg)
        torch.cuda.synchronize()
        assert np.array_equal(l1.cpu().numpy()[0], l0.cpu().numpy()) and np.array_equal(t1.cpu().numpy()[0], t0.cpu().numpy())


def test_arguments(lib, torch):
    N = 4096
    p = abi.default_params()
    pl = tspws.Plan(tspws.resolve(p, N), N)
    X = torch.zeros((20, N), dtype=torch.float32, device="cuda")
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch(X, [0, 10, 5])                 # decreasing
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch(X, [0, 10, 21])                # past the rows
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch(X, np.array([0.0, 10.0]))      # not integers
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch(X[:, :100], [0, 10])           # wrong trace length
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch(X, [0, 10, 20], ls=torch.zeros((1, N), dtype=torch.float32, device="cuda"))  # wrong output shape
    # the C entry point itself
    out = torch.zeros((2, N), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dec = np.array([0, 10, 5], dtype=np.uint64)
    ok = np.array([0, 10, 20], dtype=np.uint64)
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), X.data_ptr(), N, dec.ctypes.data, 2, out.data_ptr(), out.data_ptr(), stream) == -1
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), X.data_ptr(), N, ok.ctypes.data, 2, None, out.data_ptr(), stream) == -1
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), None, N, ok.ctypes.data, 2, out.data_ptr(), out.data_ptr(), stream) == -1
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), X.data_ptr(), N - 1, ok.ctypes.data, 2, out.data_ptr(), out.data_ptr(), stream) == -1
    assert lib.tspws_hip_stack_batch(pl.h, None, X.data_ptr(), N, ok.ctypes.data, 2, out.data_ptr(), out.data_ptr(), stream) == -1
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), X.data_ptr(), N, None, 2, out.data_ptr(), out.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert not out.any()                              # nothing was written
    # B = 0: nothing to do
    assert lib.tspws_hip_stack_batch(pl.h, C.byref(pl.params), None, N, ok.ctypes.data, 0, None, None, stream) == 0
    ls, ts = pl.stack_batch(X, [4])
    assert tuple(ls.shape) == (0, N) and tuple(ts.shape) == (0, N)
