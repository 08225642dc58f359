"""The single-stage jackknife of many ensembles in one call (tspws_hip_jackknife_batch, Plan.jackknife_batch) on the GPU: every ensemble's
replicas against the trace-order restatement (jk_single_ref.Restatement) and Plan.jackknife_single on that ensemble alone, its main rows
against the oracle and Plan.stack_single; engines pinned per process and a small scratch budget (tests/jk_batch_engine.py), refusals.
Outputs hold NaN before every call; every row with K_c > 0 is compared, every row with K_c = 0 and every empty ensemble must be exactly zero."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import jk_batch_engine as jb
import jk_single_ref as ref

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


def shared(lib, r, sizes):
    """The default engine takes the many-trace path for >= 256 traces of a frame with a spectral set: the shared pass, nothing looped."""
    st, nonempty = r["stats"], sum(1 for m in sizes if m)
    assert sum(sizes) >= 256 and lib.tspws_hip_spectral_choice(r["pl"].h, sum(sizes)) < r["pl"].S
    assert st["shared"] == nonempty and st["looped"] == 0 and st["empty"] == len(sizes) - nonempty and st["rounds"] >= 1, st


# (params, ensemble sizes, N, (n, d)): types -1 / -2 / -3, unbiased, wu = 1.3; N = 4096, 1501 and 16 501; sizes 0, 1, 40, 64, 65, 130 and 300
# in one batch (300 traces in n = 4 bins: classes of more than 64 traces, several blocks each); first[0] > 0 and ld > N (jk_batch_engine.run)
CASES = [
    (dict(), [0, 1, 40, 64, 65, 130, 300], 4096, (4, 1)),
    (dict(type=-2, unbiased=1), [65, 0, 130, 1, 64], 1501, (5, 2)),
    (dict(type=-3, wu=1.3), [64, 1, 130, 65, 0], 16501, (12, 1)),
]


@pytest.mark.parametrize("kw,sizes,N,nd", CASES)
def test_parity(lib, torch, kw, sizes, N, nd):
    r = jb.run(torch, kw, sizes, N, nd, seed=sum(sizes) + N, first0=3, pad=7)
    shared(lib, r, sizes)
    if max(sizes) >= 300:
        first, f0 = r["first"], int(r["first"][0])
        cls, _ = tspws.selection_classes(r["sel"][:, first[-2] - f0:first[-1] - f0])
        assert np.bincount(cls).max() > 64  # a class of several blocks
    e = jb.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_single_bin_ensemble(lib, torch):
    """Ensemble 0 has all its traces in bin 0 of n = 4: one class, replica 0 is empty (zero rows, count 0)."""
    sizes = [30, 100, 130]
    jan = (1262304000 + 3600 * np.arange(30)).astype(np.int64)
    times = np.concatenate([jan, jb.ensemble_times([0] + sizes[1:], 4)])
    r = jb.run(torch, dict(unbiased=1), sizes, 4096, (4, 1), seed=3, times=times)
    shared(lib, r, sizes)
    np.testing.assert_array_equal(r["jm"][0], [0, 30, 30, 30])
    assert tspws.selection_classes(r["sel"][:, :30])[1].shape[1] == 1
    e = jb.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_many_classes(lib, torch):
    """A random 0/1 selection: ~60 classes in an ensemble, more than the LDS form of the finish kernel holds; one replica keeps nothing."""
    sizes = [100, 60, 100]
    sel = (np.random.default_rng(8).random((7, sum(sizes))) < 0.55).astype(np.int8)
    sel[3, :] = 0
    assert tspws.selection_classes(sel[:, :100])[1].shape[1] > 24
    r = jb.run(torch, dict(type=-3, unbiased=1), sizes, 4096, seed=21, sel=sel)
    shared(lib, r, sizes)
    assert not r["jm"][:, 3].any()
    e = jb.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_without_main_rows(lib, torch):
    sizes = [40, 130, 0, 100]
    r = jb.run(torch, dict(wu=1.3), sizes, 4096, (5, 2), seed=9, main=False)
    shared(lib, r, sizes)
    e = jb.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_below_the_many_trace_rule(lib, torch):
    """55 traces in all: one tspws_hip_stack + tspws_hip_jackknife_single per ensemble."""
    sizes = [30, 1, 0, 24]
    r = jb.run(torch, dict(unbiased=1), sizes, 4096, (4, 1), seed=2)
    st = r["stats"]
    assert st["looped"] == 3 and st["shared"] == 0 and st["empty"] == 1 and st["pass_batches"] == 0, st
    e = jb.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


@pytest.mark.parametrize("engine", ["fir", "spectral"])
def test_engines(engine):
    env = dict(os.environ, TSPWS_ENGINE=engine)
    out = subprocess.run([sys.executable, os.path.join(HERE, "jk_batch_engine.py"), engine], capture_output=True, text=True, env=env, timeout=1500)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "JKB_DONE" in out.stdout


def test_small_budget(tmp_path):
    """The same batch with the default TSPWS_PART_MB and with 16 (several rounds; a class straddles two batches of the many-trace pass in
    both): every row matches the per-ensemble calls in the child, two calls in one process are bit-identical there, and the two runs match
    each other, to the tolerance."""
    res = {}
    for tag, extra in (("default", {}), ("small", {"TSPWS_PART_MB": "16"})):
        env = dict(os.environ)
        env.pop("TSPWS_PART_MB", None)
        env.update(extra)
        path = str(tmp_path / f"{tag}.npz")
        out = subprocess.run([sys.executable, os.path.join(HERE, "jk_batch_engine.py"), "budget", path], capture_output=True, text=True, env=env,
                             timeout=900)
        print(out.stdout[-2000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        res[tag] = np.load(path)
    np.testing.assert_array_equal(res["default"]["jm"], res["small"]["jm"])
    for k in ("ls", "ts"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            assert abi.relerr(b[r], a[r]) < TOL32, (k, r)
    for k in ("jl", "jt"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            for c in range(a.shape[1]):
                if res["default"]["jm"][r, c]:
                    assert abi.relerr(b[r, c], a[r, c]) < TOL32, (k, r, c)
                else:
                    assert not (a[r, c] != 0).any() and not (b[r, c] != 0).any(), (k, r, c)


def test_refusals(lib, torch):
    N, sizes = 4096, [10, 6]
    p = tspws.resolve(abi.default_params(), N)
    pl = tspws.Plan(p, N)
    X = torch.zeros((16, N), dtype=torch.float32, device="cuda")
    first = np.array([0, 10, 16], dtype=np.uint64)
    sel = np.ones((3, 16), np.int8)
    main = torch.full((2, 2, N), 7.0, dtype=torch.float32, device="cuda")
    rep = torch.full((2, 2, 3, N), 7.0, dtype=torch.float32, device="cuda")
    jm = np.full((2, 3), 99, np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cabi(params, ld=N, f=first, ls=main[0], ts=main[1]):
        return lib.tspws_hip_jackknife_batch(pl.h, C.byref(params), X.data_ptr(), ld, f.ctypes.data, 2, sel.ctypes.data, 3,
                                             ls.data_ptr() if ls is not None else None, ts.data_ptr() if ts is not None else None, rep[0].data_ptr(),
                                             rep[1].data_ptr(), jm.ctypes.data, stream)
    q = tspws.t_tsPWS.from_buffer_copy(pl.params)
    q.Kmax = 4  # two-stage for both ensembles (>= 4 traces)
    assert cabi(q) == -1 and b"two-stage" in lib.tspws_hip_last_error()
    assert cabi(pl.params, ld=N - 1) == -1
    assert cabi(pl.params, f=np.array([0, 10, 5], dtype=np.uint64)) == -1
    assert cabi(pl.params, ls=None) == -1
    torch.cuda.synchronize()
    assert (main == 7.0).all().item() and (rep == 7.0).all().item() and (jm == 99).all()  # outputs untouched
    # B == 0 / C == 0: nothing to do
    assert lib.tspws_hip_jackknife_batch(pl.h, C.byref(pl.params), None, N, first.ctypes.data, 0, None, 3, None, None, None, None, None, stream) == 0
    assert lib.tspws_hip_jackknife_batch(pl.h, C.byref(pl.params), None, N, first.ctypes.data, 2, None, 0, None, None, None, None, None, stream) == 0
    # the binding's own checks
    f = [0, 10, 16]
    bad = [
        lambda: pl.jackknife_batch(X.double(), f, sel),                                          # traces not float32
        lambda: pl.jackknife_batch(X, f, sel.astype(np.float64)),                                # selection not int8
        lambda: pl.jackknife_batch(X, f, sel[:, :-1]),                                           # selection of another width
        lambda: pl.jackknife_batch(X, f, sel[0]),                                                # selection not 2-D
        lambda: pl.jackknife_batch(X, [0, 10, 5], sel),                                          # decreasing offsets
        lambda: pl.jackknife_batch(X, [0, 10, 17], sel),                                         # past the rows
        lambda: pl.jackknife_batch(X, f, sel, ls=torch.zeros((1, N), device="cuda")),            # main output of the wrong shape
        lambda: pl.jackknife_batch(X, f, sel, ls_out=torch.zeros((2, 3, N + 1), device="cuda")),
        lambda: pl.jackknife_batch(X, f, sel, ts_out=torch.zeros((2, 3, N), dtype=torch.float64, device="cuda")),
        lambda: pl.jackknife_batch(X, f, sel, mtr_out=np.zeros((2, 3), np.int32)),
        lambda: pl.jackknife_batch(X, f, sel, mtr_out=np.zeros((3, 2), np.uint32)),
        lambda: pl.jackknife_batch(X, f, sel, ls=torch.zeros((2, N), device="cuda"), main=False),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(tspws.TspwsError):
            fn()
            pytest.fail(f"bad argument {k} accepted")
    ls, ts, jl, jt, m = pl.jackknife_batch(X, [4], np.ones((3, 0), np.int8))
    assert tuple(ls.shape) == (0, N) and tuple(jl.shape) == (0, 3, N) and m.shape == (0, 3)
