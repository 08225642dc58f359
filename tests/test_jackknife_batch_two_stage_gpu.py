"""The two-stage jackknife of many ensembles in one call (tspws_hip_jackknife_batch_two_stage, Plan.jackknife_batch_two_stage) on the GPU:
every ensemble's replicas and plain stack against the oracle's tspws_main on that ensemble alone with its start times and against
Plan.stack_jackknife on it (tests/jk_batch2_engine.py); a small scratch budget in child processes; refusals.  Outputs hold NaN before every
call; every row with K_c > 0 is compared, every row with K_c = 0 and every empty ensemble must be exactly zero with count 0.  The tolerance
is the batch calls' 2e-6."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import jk_batch2_engine as j2

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


def shared(r, sizes, tiles=None):
    """Two or more ensembles with traces: the shared walk, nothing looped."""
    st, nonempty = r["stats"], sum(1 for m in sizes if m)
    W = r["sel"].shape[0] + (1 if r["main"] else 0)
    assert st["shared"] == nonempty and st["looped"] == 0 and st["empty"] == len(sizes) - nonempty and st["rounds"] >= 1, st
    assert st["tiles"] == (W + 15) // 16 and st["rows"] == nonempty * W * r["p"].Kmax, st
    if tiles is not None:
        assert st["tiles"] == tiles, st


# name -> (params, ensemble sizes, N, (n, d), first0, pad)
#   A  M_b == Kmax (every group one trace) up to 300 traces; ld = N + 7: the scalar loads
#   B  Mexican hat, unbiased; 11 columns; a 12-trace ensemble whose replicas have empty groups (0 < K_c < Kmax)
#   C  ld % 4 == 0 and an aligned base: the 16-byte loads with an N % 4 == 1 tail, 17 column blocks
#   D  22 columns: two tiles
CASES = {
    "A": (dict(Kmax=4), [0, 4, 5, 40, 64, 65, 130, 300], 4096, (4, 1), 3, 7),
    "B": (dict(type=-2, unbiased=1, Kmax=10), [65, 0, 130, 10, 12], 1501, (5, 2), 2, 5),
    "C": (dict(type=-3, wu=1.3, Kmax=4), [64, 4, 130, 65, 0], 16501, (12, 1), 4, 3),
    "D": (dict(unbiased=1, Kmax=10), [40, 130, 25], 2048, (7, 2), 2, 5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity(lib, torch, name):
    kw, sizes, N, nd, first0, pad = CASES[name]
    r = j2.run(torch, kw, sizes, N, nd, seed=sum(sizes) + N, first0=first0, pad=pad)
    shared(r, sizes, tiles=2 if name == "D" else 1)
    assert r["sel"].shape[0] == abi.binomial(*nd)
    if name == "A":
        assert (N + pad) % 4 != 0
    if name == "B":
        k = r["jm"][4]
        assert ((k > 0) & (k < kw["Kmax"])).any(), k  # a replica of the 12-trace ensemble with empty groups
    if name == "C":
        assert (N + pad) % 4 == 0 and (first0 * (N + pad)) % 4 == 0 and r["buf"].data_ptr() % 16 == 0 and N % 4 == 1
    e = j2.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_single_bin_ensemble(lib, torch):
    """Ensemble 0 has all its traces in bin 0 of n = 4: replica 0 keeps nothing (zero rows, count 0)."""
    sizes = [30, 100, 130]
    jan = (1262304000 + 3600 * np.arange(30)).astype(np.int64)
    times = np.concatenate([jan, j2.ensemble_times([0] + sizes[1:], 4)])
    r = j2.run(torch, dict(unbiased=1, Kmax=10), sizes, 4096, (4, 1), seed=3, times=times)
    shared(r, sizes)
    np.testing.assert_array_equal(r["jm"][0], [0, 30, 30, 30])
    assert not (r["jl"][0, 0] != 0).any() and not (r["jt"][0, 0] != 0).any()
    e = j2.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_random_selection(lib, torch):
    """A random 0/1 selection (runs of one or two traces, groups interrupted by deleted traces); one replica keeps nothing."""
    sizes = [100, 60, 100]
    sel = (np.random.default_rng(8).random((7, sum(sizes))) < 0.55).astype(np.int8)
    sel[3, :] = 0
    r = j2.run(torch, dict(type=-3, unbiased=1, Kmax=10), sizes, 4096, seed=21, sel=sel)
    shared(r, sizes)
    assert not r["jm"][:, 3].any()
    e = j2.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32


def test_without_main_rows(lib, torch):
    sizes = [40, 130, 0, 100]
    kw = dict(wu=1.3, Kmax=10)
    r = j2.run(torch, kw, sizes, 4096, (5, 2), seed=9, main=False)
    shared(r, sizes)
    assert r["ls"] is None and r["ts"] is None
    e = j2.check(torch, r)
    print("worst relerr", e)
    assert e < TOL32
    # the replicas do not depend on the main rows being wanted (to the tolerance: the plain stack's column cuts the runs of its tile at its
    # own group ends, so the FP64 sums behind the replicas' rows may associate differently in the last bit)
    r2 = j2.run(torch, kw, sizes, 4096, (5, 2), seed=9, main=True)
    np.testing.assert_array_equal(r["jm"], r2["jm"])
    for k in ("jl", "jt"):
        for b in range(len(sizes)):
            for c in range(r["jm"].shape[1]):
                if r["jm"][b, c]:
                    assert abi.relerr(r[k][b, c], r2[k][b, c]) < TOL32, (k, b, c)
                else:
                    assert not (r[k][b, c] != 0).any() and not (r2[k][b, c] != 0).any(), (k, b, c)


def test_one_nonempty_ensemble(lib, torch):
    """The call IS Plan.stack_jackknife (main=False: tspws_hip_jackknife) for the only ensemble with traces."""
    sizes = [0, 50, 0]
    r = j2.run(torch, dict(unbiased=1, Kmax=10), sizes, 4096, (12, 1), seed=6)
    st = r["stats"]
    assert st["looped"] == 1 and st["shared"] == 0 and st["empty"] == 2 and st["rounds"] == 0, st
    f0, f1 = int(r["first"][1]), int(r["first"][2])
    seg = r["buf"][f0:f1, :r["N"]]
    sb = np.ascontiguousarray(r["sel"])
    ls, ts, jl, jt, jm = r["pl"].stack_jackknife(seg, sb)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(r["jm"][1], jm)
    for got, want in ((r["ls"][1], ls), (r["ts"][1], ts), (r["jl"][1], jl), (r["jt"][1], jt)):
        assert np.abs(got).max() > 0
        np.testing.assert_array_equal(got, want.cpu().numpy())
    for b in (0, 2):
        assert not r["jm"][b].any() and not (r["jl"][b] != 0).any() and not (r["jt"][b] != 0).any()
        assert not (r["ls"][b] != 0).any() and not (r["ts"][b] != 0).any()
    # without the main rows: tspws_hip_jackknife
    r2 = j2.run(torch, dict(unbiased=1, Kmax=10), sizes, 4096, (12, 1), seed=6, main=False)
    assert r2["stats"]["looped"] == 1
    p = r2["pl"]
    jl2 = torch.empty((sb.shape[0], r["N"]), dtype=torch.float32, device="cuda")
    jt2 = torch.empty_like(jl2)
    jm2 = np.zeros(sb.shape[0], np.uint32)
    rc = lib.tspws_hip_jackknife(p.h, C.byref(p.params), r2["buf"][f0:f1].data_ptr(), r2["buf"].shape[1], f1 - f0, sb.ctypes.data, sb.shape[0],
                                 jl2.data_ptr(), jt2.data_ptr(), jm2.ctypes.data, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(r2["jm"][1], jm2)
    np.testing.assert_array_equal(r2["jl"][1], jl2.cpu().numpy())
    np.testing.assert_array_equal(r2["jt"][1], jt2.cpu().numpy())


def test_small_budget(tmp_path):
    """The same batch with the default TSPWS_PART_MB (one round) and with 16 (several): every row matches Plan.stack_jackknife in the child,
    two calls in one process are bit-identical there, and the two runs match each other to the tolerance with identical counts."""
    res = {}
    for tag, extra in (("default", {}), ("small", {"TSPWS_PART_MB": "16"})):
        env = dict(os.environ)
        env.pop("TSPWS_PART_MB", None)
        env.update(extra)
        path = str(tmp_path / f"{tag}.npz")
        out = subprocess.run([sys.executable, os.path.join(HERE, "jk_batch2_engine.py"), "budget", path], capture_output=True, text=True, env=env,
                             timeout=900)
        print(out.stdout[-2000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "JK2_DONE" in out.stdout
        res[tag] = np.load(path)
    np.testing.assert_array_equal(res["default"]["jm"], res["small"]["jm"])
    assert res["default"]["jm"].all()
    for k in ("ls", "ts"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            assert abi.relerr(b[r], a[r]) < TOL32, (k, r)
    for k in ("jl", "jt"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            for c in range(a.shape[1]):
                assert abi.relerr(b[r, c], a[r, c]) < TOL32, (k, r, c)


def test_refusals(lib, torch):
    N = 4096
    p = tspws.resolve(abi.default_params(Kmax=4), N)
    pl = tspws.Plan(p, N)
    X = torch.zeros((36, N), dtype=torch.float32, device="cuda")
    first = np.array([0, 30, 36], dtype=np.uint64)
    sel = np.ones((3, 36), np.int8)
    main = torch.full((2, 2, N), 7.0, dtype=torch.float32, device="cuda")
    rep = torch.full((2, 2, 3, N), 7.0, dtype=torch.float32, device="cuda")
    jm = np.full((2, 3), 99, np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lib.tspws_hip_jackknife_batch_two_stage

    def cabi(params=pl.params, ld=N, f=first, ls=main[0], ts=main[1], plan=pl.h, s=sel, lo=rep[0], to=rep[1], m=jm):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return fn(plan, C.byref(params) if params is not None else None, X.data_ptr(), ld, f.ctypes.data if f is not None else None, 2,
                  s.ctypes.data if s is not None else None, 3, ptr(ls), ptr(ts), ptr(lo), ptr(to), m.ctypes.data if m is not None else None, stream)
    for kw in (dict(plan=None), dict(params=None), dict(f=None), dict(s=None), dict(lo=None), dict(to=None), dict(m=None)):
        assert cabi(**kw) == -1 and b"NULL" in lib.tspws_hip_last_error(), kw
    assert cabi(ls=None) == -1 and b"exactly one" in lib.tspws_hip_last_error()
    assert cabi(ts=None) == -1 and b"exactly one" in lib.tspws_hip_last_error()
    assert cabi(f=np.array([0, 30, 5], dtype=np.uint64)) == -1 and b"decreasing" in lib.tspws_hip_last_error()
    assert cabi(ld=N - 1) == -1 and b"stride" in lib.tspws_hip_last_error()
    q = tspws.t_tsPWS.from_buffer_copy(pl.params)
    q.Kmax = 10  # the 6-trace ensemble is single-stage
    assert cabi(params=q) == -1 and b"single-stage" in lib.tspws_hip_last_error()
    q.Kmax = 0   # no two-stage rule at all
    assert cabi(params=q) == -1 and b"single-stage" in lib.tspws_hip_last_error()
    torch.cuda.synchronize()
    assert (main == 7.0).all().item() and (rep == 7.0).all().item() and (jm == 99).all()  # outputs untouched
    # B == 0 / C == 0: nothing to do
    assert fn(pl.h, C.byref(pl.params), None, N, first.ctypes.data, 0, None, 3, None, None, None, None, None, stream) == 0
    assert fn(pl.h, C.byref(pl.params), None, N, first.ctypes.data, 2, None, 0, None, None, None, None, None, stream) == 0
    assert cabi() == 0  # (the arguments above are fine when nothing is wrong with them)
    torch.cuda.synchronize()
    assert (jm == [[30] * 3, [6] * 3]).all() and not (rep != 0).any().item() and not (main != 0).any().item()  # (zero traces: zero stacks)
    # the binding's own checks
    f = [0, 30, 36]
    call = pl.jackknife_batch_two_stage
    bad = [
        lambda: call(X.double(), f, sel),                                          # traces not float32
        lambda: call(X, f, sel.astype(np.float64)),                                # selection not int8
        lambda: call(X, f, sel[:, :-1]),                                           # selection of another width
        lambda: call(X, f, sel[0]),                                                # selection not 2-D
        lambda: call(X, [0, 30, 5], sel),                                          # decreasing offsets
        lambda: call(X, [0, 30, 37], sel),                                         # past the rows
        lambda: call(X, f, sel, ls=torch.zeros((1, N), device="cuda")),            # main output of the wrong shape
        lambda: call(X, f, sel, ls_out=torch.zeros((2, 3, N + 1), device="cuda")),
        lambda: call(X, f, sel, ts_out=torch.zeros((2, 3, N), dtype=torch.float64, device="cuda")),
        lambda: call(X, f, sel, mtr_out=np.zeros((2, 3), np.int32)),
        lambda: call(X, f, sel, mtr_out=np.zeros((3, 2), np.uint32)),
        lambda: call(X, f, sel, ls=torch.zeros((2, N), device="cuda"), main=False),
    ]
    for k, bf in enumerate(bad):
        with pytest.raises(tspws.TspwsError):
            bf()
            pytest.fail(f"bad argument {k} accepted")
    ls, ts, jl, jt, m = call(X, [4], np.ones((3, 0), np.int8))
    assert tuple(ls.shape) == (0, N) and tuple(jl.shape) == (0, 3, N) and m.shape == (0, 3)
