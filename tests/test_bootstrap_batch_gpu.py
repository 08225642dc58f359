"""Bootstrap replicas of many ensembles in one call (tspws_hip_bootstrap_batch / _cnt, Plan.bootstrap_batch) on the GPU, shipped library: the
rows of one batch (tests/boot_batch_engine.py: ensembles of 1, 3, 5, 8, 0, 67 traces, h_first[0] = 2, ld = N + 5; drawn rows, an all-zero
row, a single count of 1, count 5 on trace 0, a count of 255, an all-ones row) against the expanded-ensemble checker tests/boot_batch_ref.py in
three frames, three weight modes and M on both sides of the group of 8; the all-ones row against Plan.stack_batch; a 0/1 matrix against
Plan.subsample_batch; a repeated call; a small scratch budget in a child process; the statistics; the drawing variant; refusals.  Every
comparison of rows uses the project's parity figure, relerr <= 2e-6."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import boot_batch_engine as bbe

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


def built_as_given(r):
    """Plan.bootstrap_batch_stats() shows the batch as it was built."""
    st, M = r["stats"], r["cnt"].shape[0]
    c0, mx = 0, 0
    for mb in bbe.SIZES:  # (columns outside the ensembles do not exist here: T is the sum of the sizes)
        mx = max(mx, int(r["cnt"][:, c0:c0 + mb].max()) if mb else 0)
        c0 += mb
    assert st["shared"] == 5 and st["empty"] == 1 and st["rows"] == 5 * M and st["max_count"] == mx and st["rounds"] >= 1, st


@pytest.mark.parametrize("M", [1, 8, 9, 17])
@pytest.mark.parametrize("weight", sorted(bbe.WEIGHTS))
@pytest.mark.parametrize("frame", sorted(bbe.FRAMES))
def test_parity(lib, torch, frame, weight, M):
    r = bbe.run(torch, frame, weight, bbe.counts()[:M])
    built_as_given(r)
    if M > bbe.ROW_255:
        assert r["stats"]["max_count"] == 255
        assert not r["sm"][:, bbe.ROW_ZERO].any()
        assert (r["sm"][[0, 1, 2, 3, 5], bbe.ROW_ONE] == 1).all() and (r["sm"][[0, 1, 2, 3, 5], bbe.ROW_FIVE] == 5).all()
    assert not r["sm"][4].any() and not (r["sl"][4] != 0).any() and not (r["st"][4] != 0).any()  # the empty ensemble
    e = bbe.check(r)
    print("worst relerr", e)
    assert e <= TOL32
    if M > bbe.ROW_ONES:  # the all-ones row is the ensemble's plain ts-PWS stack
        _, ts = r["pl"].stack_batch(r["buf"][:, :r["N"]], bbe.FIRST)
        torch.cuda.synchronize()
        ts = ts.cpu().numpy()
        worst = 0.0
        for b, mb in enumerate(bbe.SIZES):
            if mb:
                assert np.abs(ts[b]).max() > 0 and r["sm"][b, bbe.ROW_ONES] == mb
                worst = max(worst, abi.relerr(r["st"][b, bbe.ROW_ONES], ts[b]))
        print("all-ones row against stack_batch: worst relerr", worst)
        assert worst <= TOL32


@pytest.mark.parametrize("weight", ["unbiased", "wu1.5"])
def test_masks_agree_with_subsample_batch(lib, torch, weight):
    """A 0/1 matrix: the rows of Plan.subsample_batch on the same matrix as masks (whether they are bit for bit is printed, and recorded in
    DESIGN.md section 18); among the rows one that keeps nothing and one that keeps a single trace."""
    M, T = 9, sum(bbe.SIZES)
    sel = (np.random.default_rng(12).random((M, T)) < 0.6).astype(np.uint8)
    sel[1, :] = 0
    sel[2, :] = 0
    sel[2, [0, 2, 6, 10, 20]] = 1
    r = bbe.run(torch, "morlet2048", weight, sel)
    built_as_given(r)
    bbe.check_counts(r)
    ls, ts, mtr = r["pl"].subsample_batch(r["buf"][:, :r["N"]], bbe.FIRST, sel.astype(np.int8))
    torch.cuda.synchronize()
    ls, ts = ls.cpu().numpy(), ts.cpu().numpy()
    np.testing.assert_array_equal(mtr, r["sm"])
    worst, n = 0.0, 0
    for b in range(len(bbe.SIZES)):
        for m in range(M):
            if mtr[b, m]:
                assert np.abs(ls[b, m]).max() > 0 and np.abs(ts[b, m]).max() > 0
                worst = max(worst, abi.relerr(r["sl"][b, m], ls[b, m]), abi.relerr(r["st"][b, m], ts[b, m]))
                n += 1
    print("0/1 matrix against subsample_batch: worst relerr", worst, "bit for bit:", bool(np.array_equal(ls, r["sl"]) and np.array_equal(ts, r["st"])))
    assert n > 30 and worst <= TOL32


def test_repeated_call_is_bit_identical(lib, torch):
    r = bbe.run(torch, "mexhat2048", "unbiased", bbe.counts(), stats=True)
    first = {k: r[k].copy() for k in ("sl", "st", "sm", "mom")}
    bbe.call(torch, r)
    for k in first:
        assert np.isfinite(r[k]).all() and np.array_equal(first[k], r[k]), k


def test_small_budget_takes_rounds_bit_identically(lib, torch, tmp_path):
    """The batch under the smallest TSPWS_PART_MB in a child process (several rounds) against the one-round run of this process, bit for bit."""
    r = bbe.run(torch, "morlet2048", "biased", bbe.counts())
    assert r["stats"]["rounds"] == 1, r["stats"]
    env = dict(os.environ, TSPWS_PART_MB="16")
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "boot_batch_engine.py"), "budget", path], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "BOOT_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) > 1
    assert (np.abs(r["st"][[0, 1, 2, 3, 5], 0]).max(axis=1) > 0).all()
    for k in ("sl", "st", "sm"):
        np.testing.assert_array_equal(small[k], r[k])


def moments(rows, K):
    """numpy FP64 mean and bootstrap standard error of float rows [M][N] over the replicas with K > 0, in replica order; as float32 [2][N]."""
    v = rows[K > 0].astype(np.float64)
    n, N = len(v), rows.shape[1]
    mean, ss = np.zeros(N), np.zeros(N)
    for x in v:
        mean = mean + x
    if n:
        mean = mean / n
    for x in v:
        ss = ss + (x - mean) * (x - mean)
    se = np.sqrt(ss / (n - 1)) if n > 1 else np.zeros(N)
    return np.stack([mean, se]).astype(np.float32)


@pytest.mark.parametrize("M", [1, 17])
def test_statistics(lib, torch, M):
    """d_stats against the numpy FP64 mean and standard error of the call's own float rows over the replicas with K > 0: relerr <= 1e-12 (FP64
    sums of at most 17 floats: error below 17 * 2^-53, with a wide margin; the float results then are the same floats).  M = 1 gives zero
    errors; an ensemble whose rows are all K = 0 and the empty ensemble give zeros.  The replicas of the one-trace ensemble are all that
    trace, so their ts-PWS rows can be the same floats and that error exactly zero: there, and only there, a zero reference is accepted."""
    cnt = bbe.counts()[:M].copy()
    cnt[:, 1:4] = 0  # ensemble 1 (3 traces): K = 0 in every row
    r = bbe.run(torch, "morlet1501", "unbiased", cnt, stats=True)
    built_as_given(r)
    bbe.check_counts(r)
    mom = r["mom"]
    assert mom.shape == (len(bbe.SIZES), 4, r["N"]) and np.isfinite(mom).all()
    assert not r["sm"][1].any() and not (mom[1] != 0).any() and not (mom[4] != 0).any()
    worst = 0.0
    for b in (0, 2, 3, 5):
        want = np.concatenate([moments(r["sl"][b], r["sm"][b]), moments(r["st"][b], r["sm"][b])])
        nrep = int((r["sm"][b] > 0).sum())
        assert nrep == (1 if M == 1 else 16)
        for q in range(4):
            if q % 2 and nrep <= 1:
                assert not (mom[b, q] != 0).any() and not (want[q] != 0).any(), (b, q)
                continue
            if np.abs(want[q]).max() > 0:
                worst = max(worst, abi.relerr(mom[b, q], want[q]))
            else:  # only the replicas of the one-trace ensemble may all be the same floats (every replica is that trace): an error of exactly zero
                assert q % 2 and bbe.SIZES[b] == 1 and not (mom[b, q] != 0).any(), (b, q)
    print("statistics: worst relerr", worst)
    assert worst <= 1e-12
    # the rows are the rows of the call without statistics
    r0 = bbe.run(torch, "morlet1501", "unbiased", cnt)
    assert r0["mom"] is None and np.array_equal(r0["sl"], r["sl"]) and np.array_equal(r0["st"], r["st"])


def test_drawing_variant(lib, torch):
    """tspws_hip_bootstrap_batch after abi.srand(s) == the _cnt call with bootstrap_counts_batch after the same seed, bit for bit."""
    abi.srand(31)
    cnt = tspws.bootstrap_counts_batch(bbe.FIRST, 3)
    r = bbe.run(torch, "morlet2048", "unbiased", cnt, stats=True)
    pl, B, M, N = r["pl"], len(bbe.SIZES), 3, r["N"]
    assert (r["sm"] == np.array(bbe.SIZES)[:, None]).all()
    sl = torch.full((B, M, N), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((B, M, N), float("nan"), dtype=torch.float32, device="cuda")
    mo = torch.full((B, 4, N), float("nan"), dtype=torch.float32, device="cuda")
    sm = np.full((B, M), 99, np.uint32)
    f = np.ascontiguousarray(bbe.FIRST, dtype=np.uint64)
    abi.srand(31)
    rc = lib.tspws_hip_bootstrap_batch(pl.h, C.byref(pl.params), r["buf"].data_ptr(), r["buf"].shape[1], f.ctypes.data, B, M, sl.data_ptr(), st.data_ptr(),
                                       sm.ctypes.data, mo.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tspws_hip_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sm, r["sm"])
    assert (np.abs(r["st"][[0, 1, 2, 3, 5]]).max(axis=2) > 0).all()
    np.testing.assert_array_equal(sl.cpu().numpy(), r["sl"])
    np.testing.assert_array_equal(st.cpu().numpy(), r["st"])
    np.testing.assert_array_equal(mo.cpu().numpy(), r["mom"])


def test_refusals(lib, torch):
    N, M = 2048, 4  # (M = 4: a block of 2 M N floats holds the [2][4][N] statistics)
    p = tspws.resolve(abi.default_params(Kmax=10), N)
    pl = tspws.Plan(p, N)
    X = torch.zeros((9, N), dtype=torch.float32, device="cuda")
    first = np.array([0, 6, 9], dtype=np.uint64)
    cnt = np.ones((M, 9), np.uint8)
    rep = torch.full((3, 2, M, N), 7.0, dtype=torch.float32, device="cuda")  # ls_out, ts_out and the statistics
    sm = np.full((2, M), 99, np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    two = tspws.resolve(abi.default_params(Kmax=2), N)  # Kmax = 2 <= 6 and 3 traces: two-stage

    def cabi(drawing, params=pl.params, x=X, ld=N, f=first, plan=pl.h, c=cnt, lo=rep[0], to=rep[1], m=sm, B=2, Mn=M):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        head = (plan, C.byref(params) if params is not None else None, ptr(x), ld, f.ctypes.data if f is not None else None, B, Mn)
        tail = (ptr(lo), ptr(to), m.ctypes.data if m is not None else None, rep[2].data_ptr(), stream)
        abi.srand(5)
        r0 = C.CDLL(None).rand()
        abi.srand(5)
        if drawing:
            rc = lib.tspws_hip_bootstrap_batch(*head, *tail)
        else:
            rc = lib.tspws_hip_bootstrap_batch_cnt(*head, c.ctypes.data if c is not None else None, *tail)
        if rc:
            assert C.CDLL(None).rand() == r0  # a refused call draws nothing
        return rc
    for drawing in (False, True):
        nulls = [dict(plan=None), dict(params=None), dict(f=None), dict(lo=None), dict(to=None), dict(m=None), dict(x=None)] + ([] if drawing else [dict(c=None)])
        for kw in nulls:
            assert cabi(drawing, **kw) == -1 and b"bootstrap_batch: NULL" in lib.tspws_hip_last_error(), kw
        assert cabi(drawing, f=np.array([0, 6, 5], dtype=np.uint64)) == -1 and b"bootstrap_batch: decreasing" in lib.tspws_hip_last_error()
        assert cabi(drawing, ld=N - 1) == -1 and b"bootstrap_batch: row stride" in lib.tspws_hip_last_error()
        # a two-stage parameter set: Kmax = 2, ensembles of 5 and 4 traces
        assert cabi(drawing, params=two, f=np.array([0, 5, 9], dtype=np.uint64)) == -1
        assert b"bootstrap_batch: " in lib.tspws_hip_last_error() and b"two-stage" in lib.tspws_hip_last_error()
        torch.cuda.synchronize()
        assert (rep == 7.0).all().item() and (sm == 99).all()  # outputs untouched
        # B == 0 / M == 0: nothing to do
        assert cabi(drawing, B=0) == 0 and cabi(drawing, Mn=0) == 0
        torch.cuda.synchronize()
        assert (rep == 7.0).all().item() and (sm == 99).all()
    with pytest.raises(tspws.TspwsError, match="two-stage"):
        tspws.Plan(two, N).bootstrap_batch(X, [0, 5, 9], cnt)
    assert cabi(False) == 0  # (the arguments above are fine when nothing is wrong with them)
    torch.cuda.synchronize()
    assert (sm == [[6] * M, [3] * M]).all() and not (rep != 0).any().item()  # (zero traces: zero stacks and statistics)
    st = pl.bootstrap_batch_stats()
    assert st == dict(shared=2, empty=0, rounds=1, rows=2 * M, max_count=1), st
    # the binding's own checks
    f = [0, 6, 9]
    call = pl.bootstrap_batch
    bad = [
        lambda: call(X.double(), f, cnt),                                          # traces not float32
        lambda: call(X, f, cnt.astype(np.int8)),                                   # counts not uint8
        lambda: call(X, f, cnt[:, :-1]),                                           # counts of another width
        lambda: call(X, f, cnt[0]),                                                # counts not 2-D
        lambda: call(X, [0, 6, 5], cnt),                                           # decreasing offsets
        lambda: call(X, [0, 6, 10], cnt),                                          # past the rows
        lambda: call(X, f, cnt, ls_out=torch.zeros((2, M, N + 1), device="cuda")),
        lambda: call(X, f, cnt, ts_out=torch.zeros((2, M, N), dtype=torch.float64, device="cuda")),
        lambda: call(X, f, cnt, mtr_out=np.zeros((2, M), np.int32)),
        lambda: call(X, f, cnt, mtr_out=np.zeros((M, 2), np.uint32)),
    ]
    for k, bf in enumerate(bad):
        with pytest.raises(tspws.TspwsError):
            bf()
            pytest.fail(f"bad argument {k} accepted")
    sl, st2, m, mo = call(X, [4], np.ones((M, 0), np.uint8), stats=True)
    assert tuple(sl.shape) == (0, M, N) and m.shape == (0, M) and tuple(mo.shape) == (0, 4, N)
