"""Random subsamples of many ensembles in one call (tspws_hip_subsample_batch / _sel, Plan.subsample_batch) on the GPU: every ensemble's
block against the oracle's tspws_main on that ensemble alone (same rand() state) and against Plan.subsample_sel on it
(tests/sub_batch_engine.py); arbitrary masks row by row; one non-empty ensemble; a small scratch budget in child processes; the drawing
variant; refusals.  Outputs hold NaN (counts 99) before every call.  The tolerance is the batch calls' 2e-6."""
import ctypes as C
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import sub_batch_engine as sbe

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


def kinds(kw, sizes):
    """(single-stage, two-stage, empty) ensemble counts by the single call's rule: two-stage iff 0 < Kmax <= M_b."""
    KM = kw.get("Kmax", 0)
    two = sum(1 for m in sizes if m and KM and KM <= m)
    return sum(1 for m in sizes if m) - two, two, sum(1 for m in sizes if not m)


def shared(r):
    st = r["stats"]
    n1, n2, n0 = kinds(r["kw"], r["sizes"])
    assert st["single_shared"] == n1 and st["two_stage_shared"] == n2 and st["empty"] == n0 and st["looped"] == 0, st
    assert st["rows"] == (n1 + n2) * r["M"] and st["rounds"] >= (n1 > 0) + (n2 > 0), st


# name -> (params, ensemble sizes, N, M, p, first0, pad)
#   A  single-stage only: the 4-trace unroll tail, ensemble borders inside a forward batch of 64 traces, a second mask group with one mask,
#      ld = N + 7 (scalar loads)
#   B  type = -3, unbiased, odd N, ld % 4 == 0
#   C  both kinds in one batch (Kmax = 10): three mask groups, two column tiles of the walk
CASES = {
    "A": (dict(), [0, 1, 3, 4, 5, 63, 64, 65, 130], 4096, 9, 0.5, 3, 7),
    "B": (dict(type=-3, unbiased=1), [65, 0, 30, 2], 1501, 3, 0.7, 2, 3),
    "C": (dict(Kmax=10, unbiased=1), [4, 10, 9, 40, 0, 130, 12], 2048, 17, 0.6, 2, 5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity(lib, torch, name):
    kw, sizes, N, M, prob, first0, pad = CASES[name]
    seeds = [1000 * (ord(name) - 64) + b for b in range(len(sizes))]
    r = sbe.run(torch, kw, sizes, N, sbe.draw(sizes, M, prob, seeds), prob=prob, seed=sum(sizes) + N, first0=first0, pad=pad)
    shared(r)
    if name == "A":
        assert (N + pad) % 4 != 0 and kinds(kw, sizes)[1] == 0
    if name == "B":
        assert (N + pad) % 4 == 0
    if name == "C":
        n1, n2, _ = kinds(kw, sizes)
        assert n1 == 2 and n2 == 4 and (M + 7) // 8 == 3 and (M + 15) // 16 == 2
    e = sbe.check(torch, r, seeds)
    print("worst relerr", e)
    assert e < TOL32


def test_all_traces_kept_is_the_plain_stack(lib, torch):
    """D: p = 1.0, single-stage: every ts-PWS subsample of an ensemble is its plain stack.  (The linear rows are not compared: the plain
    stack's ls is a reconstruction through the frame, the subsample's a time-domain sum; check() below holds them to their own references.)"""
    sizes, N, M = [5, 0, 33, 1, 70], 4096, 3
    seeds = [40 + b for b in range(len(sizes))]
    r = sbe.run(torch, dict(unbiased=1), sizes, N, sbe.draw(sizes, M, 1.0, seeds), prob=1.0, seed=17)
    shared(r)
    assert (r["sel"] == 1).all()
    _, ts = r["pl"].stack_batch(r["buf"][:, :N], r["first"])
    torch.cuda.synchronize()
    ts = ts.cpu().numpy()
    worst = 0.0
    for b, seg, sb in sbe.blocks(r):
        assert np.abs(ts[b]).max() > 0
        for m in range(M):
            worst = max(worst, abi.relerr(r["st"][b, m], ts[b]))
    print("worst relerr", worst)
    assert worst < TOL32
    assert sbe.check(torch, r, seeds) < TOL32


def test_arbitrary_masks(lib, torch):
    """E: a given random 0/1 matrix; a row that keeps nothing in a single-stage and in a two-stage ensemble, a row that keeps exactly one trace
    (the K = 1 rule of the unbiased weight), a two-stage row with 0 < K < Kmax (empty groups)."""
    kw, sizes, N, M = dict(Kmax=10, unbiased=1), [25, 7, 0, 12, 3], 2048, 5
    sel = (np.random.default_rng(8).random((M, sum(sizes))) < 0.55).astype(np.int8)
    sel[0, 0:25] = 0                  # ensemble 0 (two-stage), row 0: nothing
    sel[1, 25:32] = 0                 # ensemble 1 (single-stage), row 1: nothing
    sel[2, 25:32] = 0
    sel[2, 28] = 1                    # ... row 2: exactly one trace
    sel[3, 32:44] = 0
    sel[3, [33, 36, 40, 43]] = 1      # ensemble 3 (two-stage), row 3: 4 of 12 traces, Kmax = 10
    r = sbe.run(torch, kw, sizes, N, sel, seed=23)
    shared(r)
    assert r["sm"][0, 0] == 0 and r["sm"][1, 1] == 0 and r["sm"][1, 2] == 1 and r["sm"][3, 3] == 4
    for b, m in ((0, 0), (1, 1)):
        assert not (r["sl"][b, m] != 0).any() and not (r["st"][b, m] != 0).any()
    e = sbe.check_rows(torch, r)
    print("worst relerr", e)
    assert e < TOL32


@pytest.mark.parametrize("kw,m", [(dict(unbiased=1), 50), (dict(unbiased=1, Kmax=10), 50)])
def test_one_nonempty_ensemble(lib, torch, kw, m):
    """F: the call IS Plan.subsample_sel for the only ensemble with traces."""
    sizes, N, M, prob = [0, m, 0], 4096, 5, 0.5
    seeds = [7, 8, 9]
    r = sbe.run(torch, kw, sizes, N, sbe.draw(sizes, M, prob, seeds), prob=prob, seed=6)
    st = r["stats"]
    assert st["looped"] == 1 and st["single_shared"] == 0 and st["two_stage_shared"] == 0 and st["empty"] == 2 and st["rounds"] == 0 and st["rows"] == M, st
    f0, f1 = int(r["first"][1]), int(r["first"][2])
    ls, ts = r["pl"].subsample_sel(r["buf"][f0:f1, :N], np.ascontiguousarray(r["sel"]))
    torch.cuda.synchronize()
    assert (r["sm"][1] == math.ceil(m * prob)).all()
    for got, want in ((r["sl"][1], ls), (r["st"][1], ts)):
        assert (np.abs(got).max(axis=1) > 0).all()
        np.testing.assert_array_equal(got, want.cpu().numpy())
    for b in (0, 2):
        assert not r["sm"][b].any() and not (r["sl"][b] != 0).any() and not (r["st"][b] != 0).any()
    assert sbe.check(torch, r, seeds) < TOL32


def test_small_budget(tmp_path):
    """G: the same batch with the default TSPWS_PART_MB (one round) and with 16 (several): every block matches Plan.subsample_sel in the child,
    two calls in one process are bit-identical there, and the two runs match each other to the tolerance with identical counts."""
    res = {}
    for tag, extra in (("default", {}), ("small", {"TSPWS_PART_MB": "16"})):
        env = dict(os.environ)
        env.pop("TSPWS_PART_MB", None)
        env.update(extra)
        path = str(tmp_path / f"{tag}.npz")
        out = subprocess.run([sys.executable, os.path.join(HERE, "sub_batch_engine.py"), "budget", path], capture_output=True, text=True, env=env,
                             timeout=900)
        print(out.stdout[-2000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        assert "SUB_DONE" in out.stdout
        res[tag] = np.load(path)
    np.testing.assert_array_equal(res["default"]["sm"], res["small"]["sm"])
    assert res["default"]["sm"].all()
    for k in ("sl", "st"):
        a, b = res["default"][k], res["small"][k]
        for r in range(a.shape[0]):
            for c in range(a.shape[1]):
                assert np.abs(a[r, c]).max() > 0
                assert abi.relerr(b[r, c], a[r, c]) < TOL32, (k, r, c)


def test_drawing_variant(lib, torch):
    """H: tspws_hip_subsample_batch after abi.srand(s) == the _sel call with subsampling_selection_batch after the same seed, bit for bit."""
    kw, sizes, N, M, prob = dict(Kmax=10, unbiased=1), [6, 0, 20, 9], 2048, 4, 0.5
    first = sbe.offsets(sizes, 2)
    abi.srand(31)
    sel = tspws.subsampling_selection_batch(first, M, prob)
    r = sbe.run(torch, kw, sizes, N, sel, prob=prob, seed=3)
    shared(r)
    pl, B = r["pl"], len(sizes)
    sl = torch.full((B, M, N), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((B, M, N), float("nan"), dtype=torch.float32, device="cuda")
    sm = np.full((B, M), 99, np.uint32)
    f = np.ascontiguousarray(first, dtype=np.uint64)
    abi.srand(31)
    rc = lib.tspws_hip_subsample_batch(pl.h, C.byref(pl.params), r["buf"].data_ptr(), r["buf"].shape[1], f.ctypes.data, B, M, sl.data_ptr(), st.data_ptr(),
                                       sm.ctypes.data, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tspws_hip_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sm, r["sm"])
    assert (np.abs(r["st"][[0, 2, 3]]).max(axis=2) > 0).all()
    np.testing.assert_array_equal(sl.cpu().numpy(), r["sl"])
    np.testing.assert_array_equal(st.cpu().numpy(), r["st"])


def test_refusals(lib, torch):
    N, M = 4096, 3
    p = tspws.resolve(abi.default_params(Kmax=10, subsmpl_N=M, subsmpl_p=0.5), N)
    pl = tspws.Plan(p, N)
    X = torch.zeros((36, N), dtype=torch.float32, device="cuda")
    first = np.array([0, 30, 36], dtype=np.uint64)
    sel = np.ones((M, 36), np.int8)
    rep = torch.full((2, 2, M, N), 7.0, dtype=torch.float32, device="cuda")
    sm = np.full((2, M), 99, np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cabi(drawing, params=pl.params, x=X, ld=N, f=first, plan=pl.h, s=sel, lo=rep[0], to=rep[1], m=sm, B=2, Mn=M):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        head = (plan, C.byref(params) if params is not None else None, ptr(x), ld, f.ctypes.data if f is not None else None, B, Mn)
        tail = (ptr(lo), ptr(to), m.ctypes.data if m is not None else None, stream)
        if drawing:
            return lib.tspws_hip_subsample_batch(*head, *tail)
        return lib.tspws_hip_subsample_batch_sel(*head, s.ctypes.data if s is not None else None, *tail)
    for drawing in (False, True):
        nulls = [dict(plan=None), dict(params=None), dict(f=None), dict(lo=None), dict(to=None), dict(m=None), dict(x=None)] + ([] if drawing else [dict(s=None)])
        for kw in nulls:
            assert cabi(drawing, **kw) == -1 and b"subsample_batch: NULL" in lib.tspws_hip_last_error(), kw
        assert cabi(drawing, f=np.array([0, 30, 5], dtype=np.uint64)) == -1 and b"subsample_batch: decreasing" in lib.tspws_hip_last_error()
        assert cabi(drawing, ld=N - 1) == -1 and b"subsample_batch: row stride" in lib.tspws_hip_last_error()
        torch.cuda.synchronize()
        assert (rep == 7.0).all().item() and (sm == 99).all()  # outputs untouched
        # B == 0 / M == 0: nothing to do
        assert cabi(drawing, B=0) == 0 and cabi(drawing, Mn=0) == 0
        torch.cuda.synchronize()
        assert (rep == 7.0).all().item() and (sm == 99).all()
    assert cabi(False) == 0  # (the arguments above are fine when nothing is wrong with them)
    torch.cuda.synchronize()
    assert (sm == [[30] * M, [6] * M]).all() and not (rep != 0).any().item()  # (zero traces: zero stacks)
    st = pl.subsample_batch_stats()
    assert st["single_shared"] == 1 and st["two_stage_shared"] == 1 and st["looped"] == 0, st
    # the binding's own checks
    f = [0, 30, 36]
    call = pl.subsample_batch
    bad = [
        lambda: call(X.double(), f, sel),                                          # traces not float32
        lambda: call(X, f, sel.astype(np.float64)),                                # masks not int8
        lambda: call(X, f, sel[:, :-1]),                                           # masks of another width
        lambda: call(X, f, sel[0]),                                                # masks not 2-D
        lambda: call(X, [0, 30, 5], sel),                                          # decreasing offsets
        lambda: call(X, [0, 30, 37], sel),                                         # past the rows
        lambda: call(X, f, sel, ls_out=torch.zeros((2, M, N + 1), device="cuda")),
        lambda: call(X, f, sel, ts_out=torch.zeros((2, M, N), dtype=torch.float64, device="cuda")),
        lambda: call(X, f, sel, mtr_out=np.zeros((2, M), np.int32)),
        lambda: call(X, f, sel, mtr_out=np.zeros((M, 2), np.uint32)),
    ]
    for k, bf in enumerate(bad):
        with pytest.raises(tspws.TspwsError):
            bf()
            pytest.fail(f"bad argument {k} accepted")
    sl, st2, m = call(X, [4], np.ones((M, 0), np.int8))
    assert tuple(sl.shape) == (0, M, N) and m.shape == (0, M)
