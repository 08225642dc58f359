"""Real-weighted stacks of many ensembles in one call (tspws_hip_weighted_stack_batch, Plan.weighted_stack_batch) on the GPU, shipped library:
the rows of one batch (tests/weighted_batch_engine.py: ensembles of 1, 3, 5, 8, 0, 67 traces, h_first[0] = 2, ld = N + 5; random rows with
exact zeros, an all-zero row, a single weight, all ones, all 0.25, a 0/1 row, a row spanning 1e-6 .. 1e6) against the checker
tests/weighted_batch_ref.py in three frames, three weight modes and M on both sides of the group of 8; a 0/1 matrix against
Plan.subsample_batch, bit for bit; the all-ones row against Plan.stack_batch; power-of-two scalings, bit for bit; integer rows against
Plan.bootstrap_batch; a repeated call; a small scratch budget in a child process; scores to weights to stacks end to end; refusals.  Every
comparison of rows that is not bit for bit uses the project's parity figure, relerr <= 2e-6."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import boot_batch_engine as bbe
import weighted_batch_engine as wbe
import weighted_batch_ref as wbr

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
    """Plan.weighted_stack_batch_stats() shows the batch as it was built."""
    st, M = r["stats"], r["w"].shape[0]
    assert st["shared"] == 5 and st["empty"] == 1 and st["rows"] == 5 * M and st["rounds"] >= 1 and len(st) == 4, st


@pytest.mark.parametrize("M", [1, 8, 9, 17])
@pytest.mark.parametrize("weight", sorted(wbe.WEIGHTS))
@pytest.mark.parametrize("frame", sorted(wbe.FRAMES))
def test_parity(lib, torch, frame, weight, M):
    r = wbe.run(torch, frame, weight, wbe.weights()[:M])
    built_as_given(r)
    if M > wbe.ROW_WIDE:
        assert not r["sm"][:, wbe.ROW_ZERO].any() and not r["keff"][:, wbe.ROW_ZERO].any()
        assert (r["sm"][wbe.NONEMPTY, wbe.ROW_ONE] == 1).all() and (r["keff"][wbe.NONEMPTY, wbe.ROW_ONE] == 1).all()
        for row in (wbe.ROW_ONES, wbe.ROW_QUARTER, wbe.ROW_WIDE):
            np.testing.assert_array_equal(r["sm"][:, row], wbe.SIZES)
        for row in (wbe.ROW_ONES, wbe.ROW_QUARTER):  # equal weights that are powers of two: Keff = n+ exactly
            np.testing.assert_array_equal(r["keff"][:, row], wbe.SIZES)
    assert not r["sm"][4].any() and not r["keff"][4].any() and not (r["sl"][4] != 0).any() and not (r["st"][4] != 0).any()  # the empty ensemble
    e = wbe.check(r)
    print("worst relerr", e)
    assert e <= TOL32
    if M > wbe.ROW_QUARTER:
        # the all-ones row is the ensemble's plain ts-PWS stack
        _, ts = r["pl"].stack_batch(r["buf"][:, :r["N"]], wbe.FIRST)
        torch.cuda.synchronize()
        ts = ts.cpu().numpy()
        worst = 0.0
        for b in wbe.NONEMPTY:
            assert np.abs(ts[b]).max() > 0
            worst = max(worst, abi.relerr(r["st"][b, wbe.ROW_ONES], ts[b]))
        print("all-ones row against stack_batch: worst relerr", worst)
        assert worst <= TOL32
        # ... and the all-0.25 row is the all-ones row, bit for bit
        np.testing.assert_array_equal(r["sl"][:, wbe.ROW_QUARTER], r["sl"][:, wbe.ROW_ONES])
        np.testing.assert_array_equal(r["st"][:, wbe.ROW_QUARTER], r["st"][:, wbe.ROW_ONES])


@pytest.mark.parametrize("weight", ["unbiased", "wu1.5"])
def test_masks_are_subsample_batch_bit_for_bit(lib, torch, weight):
    """A 0/1 matrix (the one of tests/test_bootstrap_batch_gpu.py's mask test, as float64): ls, ts and the counts of Plan.subsample_batch on the
    same matrix as masks, bit for bit; among the rows one that keeps nothing and one that keeps a single trace."""
    M, T = 9, sum(wbe.SIZES)
    sel = (np.random.default_rng(12).random((M, T)) < 0.6).astype(np.uint8)
    sel[1, :] = 0
    sel[2, :] = 0
    sel[2, [0, 2, 6, 10, 20]] = 1
    r = wbe.run(torch, "morlet2048", weight, sel.astype(np.float64))
    built_as_given(r)
    wbe.check_counts(r)
    ls, ts, mtr = r["pl"].subsample_batch(r["buf"][:, :r["N"]], wbe.FIRST, sel.astype(np.int8))
    torch.cuda.synchronize()
    ls, ts = ls.cpu().numpy(), ts.cpu().numpy()
    np.testing.assert_array_equal(mtr, r["sm"])
    np.testing.assert_array_equal(r["keff"], mtr.astype(np.float64))
    n = sum(1 for b in range(len(wbe.SIZES)) for m in range(M) if mtr[b, m] and np.abs(ls[b, m]).max() > 0 and np.abs(ts[b, m]).max() > 0)
    assert n > 30 and n == int((mtr > 0).sum())
    d = np.argwhere((ls != r["sl"]) | (ts != r["st"]))
    print("0/1 matrix against subsample_batch: differing (b, m) rows", sorted({(int(b), int(m)) for b, m, _ in d}))
    np.testing.assert_array_equal(r["sl"], ls)
    np.testing.assert_array_equal(r["st"], ts)


@pytest.mark.parametrize("weight", sorted(wbe.WEIGHTS))
def test_power_of_two_scaling_is_bit_identical(lib, torch, weight):
    """A whole matrix times 0.25: the same bits (every product, sum and quotient of the definition scales exactly)."""
    r = wbe.run(torch, "morlet1501", weight, wbe.weights())
    a = {k: r[k].copy() for k in ("sl", "st", "sm", "keff")}
    assert (np.abs(a["st"][wbe.NONEMPTY, 0]).max(axis=1) > 0).all()
    r = wbe.run(torch, "morlet1501", weight, 0.25 * wbe.weights())
    for k in a:
        np.testing.assert_array_equal(r[k], a[k], err_msg=k)


INTEGER_MAX = 32


@pytest.mark.parametrize("weight", ["biased", "wu1.5"])
def test_integer_rows_agree_with_bootstrap_batch(lib, torch, weight):
    """Integer rows as weights against Plan.bootstrap_batch on the same counts, biased modes only (the unbiased estimators differ by
    design: Keff = (sum c)^2 / sum c^2 here, K = sum c there): every row, ls and ts, relerr <= 2e-6 -- this call multiplies where that one
    adds repeatedly.  The counts are the matrix of tests/boot_batch_engine.py (drawn rows, an empty row, single counts of 1 and 5) with its
    planted count of 255 lowered to 32: the ls rows are FLOAT accumulators, the counted call rounds to float after each of the c copies of
    a trace and this call after one product, up to (c - 1) 2^-25 relative between them -- 9.2e-7 at c = 32, above the figure from c = 65
    on whatever either call does -- so the comparison keeps its counts where the figure can hold."""
    cnt = bbe.counts().copy()
    assert int(cnt[bbe.ROW_255].max()) == 255
    cnt[cnt > INTEGER_MAX] = INTEGER_MAX
    assert int(cnt.max()) == INTEGER_MAX and (cnt.max(axis=1) > 1).sum() >= 10
    r = wbe.run(torch, "mexhat2048", weight, cnt.astype(np.float64))
    wbe.check_counts(r)
    ls, ts, K = r["pl"].bootstrap_batch(r["buf"][:, :r["N"]], wbe.FIRST, cnt)
    torch.cuda.synchronize()
    ls, ts = ls.cpu().numpy(), ts.cpu().numpy()
    worst, n = 0.0, 0
    for b in wbe.NONEMPTY:
        for m in range(len(cnt)):
            assert (K[b, m] > 0) == (r["sm"][b, m] > 0)
            if K[b, m]:
                assert np.abs(ls[b, m]).max() > 0 and np.abs(ts[b, m]).max() > 0
                el, et = abi.relerr(r["sl"][b, m], ls[b, m]), abi.relerr(r["st"][b, m], ts[b, m])
                print(f"  ensemble {b} row {m} (largest count {int(cnt[m].max())}): relerr ls {el:.3e} ts {et:.3e}")
                worst = max(worst, el, et)
                n += 1
    print("integer rows against bootstrap_batch: worst relerr", worst)
    assert n == 5 * 16 and worst <= TOL32


def test_keff_of_exactly_one_takes_the_k1_rule(lib, torch):
    """Unbiased weight, one trace with weight 1 and the others with 1e-20: n+ > 1 but W = Q = Keff = 1 in FP64, so that 1 / (Keff - 1) would
    be infinite.  The row takes the K = 1 rule: finite rows equal to the checker's, which are those of the dominant trace alone."""
    T = sum(wbe.SIZES)
    w = np.full((2, T), 1e-20)
    c0 = 0
    for mb in wbe.SIZES:
        if mb:
            w[:, c0 + mb // 2] = 1.0
            w[1, c0:c0 + mb] = np.where(w[1, c0:c0 + mb] == 1.0, 1.0, 0.0)  # row 1: the dominant trace alone
        c0 += mb
    frame, weight = "morlet2048", "unbiased"
    r = wbe.run(torch, frame, weight, w)
    np.testing.assert_array_equal(r["sm"][:, 0], wbe.SIZES)
    assert (r["keff"][wbe.NONEMPTY] == 1.0).all()
    want = wbr.expected(wbe.params(frame, weight), wbe.traces(frame), wbe.FIRST, w)
    e = wbe.check(r, want)
    print("worst relerr", e)
    assert e <= TOL32
    for b in wbe.NONEMPTY:
        assert abi.relerr(r["st"][b, 0], r["st"][b, 1]) <= TOL32 and abi.relerr(r["sl"][b, 0], r["sl"][b, 1]) <= TOL32


def test_repeated_call_is_bit_identical(lib, torch):
    r = wbe.run(torch, "mexhat2048", "unbiased", wbe.weights())
    first = {k: r[k].copy() for k in ("sl", "st", "sm", "keff")}
    wbe.call(torch, r)
    for k in first:
        assert np.isfinite(r[k]).all() and np.array_equal(first[k], r[k]), k


def test_small_budget_takes_rounds_bit_identically(lib, torch, tmp_path):
    """The batch under the smallest TSPWS_PART_MB in a child process (several rounds) against the one-round run of this process, bit for bit."""
    r = wbe.run(torch, "morlet2048", "biased", wbe.weights())
    assert r["stats"]["rounds"] == 1, r["stats"]
    env = dict(os.environ, TSPWS_PART_MB="16")
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "weighted_batch_engine.py"), "budget", path], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "WEIGHTED_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) > 1
    assert (np.abs(r["st"][wbe.NONEMPTY, 0]).max(axis=1) > 0).all()
    for k in ("sl", "st", "sm", "keff"):
        np.testing.assert_array_equal(small[k], r[k])


def test_scores_to_weights_to_stacks(lib, torch):
    """End to end: stack_batch -> trace_scores against the ls row -> weights_from_scores (similarity squared; inverse energy) as two rows of
    one call.  One trace of the 8-trace ensemble is dead (zeros): its similarity is NaN, its energy 0, its weight 0 under both rules."""
    frame, weight = "morlet2048", "unbiased"
    pl, own = wbe.plan_of(torch, frame, weight)
    N = wbe.FRAMES[frame][1]
    dead = int(wbe.FIRST[3]) + 5
    buf = own.clone()
    buf[dead] = 0
    X = wbe.traces(frame).copy()
    X[dead] = 0
    ls, _ = pl.stack_batch(buf[:, :N], wbe.FIRST)
    scores, energy = pl.trace_scores(buf[:, :N], wbe.FIRST, ls.reshape(len(wbe.SIZES), 1, N), energy=True)
    torch.cuda.synchronize()
    sim, energy = scores[0, 0].cpu().numpy(), energy.cpu().numpy()
    col = dead - int(wbe.FIRST[0])
    assert np.isnan(sim[col]) and energy[col] == 0 and np.isfinite(np.delete(sim, col)).all()
    w = np.stack([tspws.weights_from_scores(sim, wbe.FIRST, "power", 2.0), tspws.weights_from_scores(energy, wbe.FIRST, "inverse", 0.0)])
    assert not w[:, col].any() and np.isfinite(w).all() and (w >= 0).all() and (w[1] <= 1).all()
    r = wbe.run(torch, frame, weight, w, buf=buf)
    built_as_given(r)
    want = wbr.expected(wbe.params(frame, weight), X, wbe.FIRST, w)
    assert (r["sm"][3] == 7).all() and (want[2][3] == 7).all()
    for b in wbe.NONEMPTY:
        for k in ("sl", "st"):
            assert np.isfinite(r[k][b]).all() and (np.abs(r[k][b]).max(axis=1) > 0).all(), (b, k)
    e = wbe.check(r, want)
    print("worst relerr", e)
    assert e <= TOL32


def test_refusals(lib, torch):
    N, M = 2048, 4
    p = tspws.resolve(abi.default_params(Kmax=10), N)
    pl = tspws.Plan(p, N)
    X = torch.zeros((9, N), dtype=torch.float32, device="cuda")
    first = np.array([0, 6, 9], dtype=np.uint64)
    w = np.ones((M, 9), np.float64)
    rep = torch.full((2, 2, M, N), 7.0, dtype=torch.float32, device="cuda")  # ls_out and ts_out
    sm = np.full((2, M), 99, np.uint32)
    ke = np.full((2, M), 7.5, np.float64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    two = tspws.resolve(abi.default_params(Kmax=2), N)  # Kmax = 2 <= 6 and 3 traces: two-stage

    def cabi(params=pl.params, x=X, ld=N, f=first, plan=pl.h, c=w, lo=rep[0], to=rep[1], m=sm, B=2, Mn=M, k=ke):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return lib.tspws_hip_weighted_stack_batch(plan, C.byref(params) if params is not None else None, ptr(x), ld, f.ctypes.data if f is not None else None, B, Mn,
                                                  c.ctypes.data if c is not None else None, ptr(lo), ptr(to), m.ctypes.data if m is not None else None,
                                                  k.ctypes.data if k is not None else None, stream)

    def bad_weight(v, row=1, col=7):
        b = w.copy()
        b[row, col] = v
        return b
    for kw in [dict(plan=None), dict(params=None), dict(f=None), dict(lo=None), dict(to=None), dict(m=None), dict(x=None), dict(c=None)]:
        assert cabi(**kw) == -1 and b"weighted_stack_batch: NULL" in lib.tspws_hip_last_error(), kw
    assert cabi(f=np.array([0, 6, 5], dtype=np.uint64)) == -1 and b"weighted_stack_batch: decreasing" in lib.tspws_hip_last_error()
    assert cabi(ld=N - 1) == -1 and b"weighted_stack_batch: row stride" in lib.tspws_hip_last_error()
    # a two-stage parameter set: Kmax = 2, ensembles of 5 and 4 traces
    assert cabi(params=two, f=np.array([0, 5, 9], dtype=np.uint64)) == -1
    assert b"weighted_stack_batch: " in lib.tspws_hip_last_error() and b"two-stage" in lib.tspws_hip_last_error()
    for v in (float("nan"), -1.0, float("inf")):
        assert cabi(c=bad_weight(v)) == -1
        assert b"weighted_stack_batch: " in lib.tspws_hip_last_error() and b"weight" in lib.tspws_hip_last_error(), v
    assert cabi(c=bad_weight(1e200)) == -1 and b"not finite" in lib.tspws_hip_last_error()
    torch.cuda.synchronize()
    assert (rep == 7.0).all().item() and (sm == 99).all() and (ke == 7.5).all()  # outputs untouched
    # B == 0 / M == 0: nothing to do
    assert cabi(B=0) == 0 and cabi(Mn=0) == 0
    torch.cuda.synchronize()
    assert (rep == 7.0).all().item() and (sm == 99).all() and (ke == 7.5).all()
    with pytest.raises(tspws.TspwsError, match="two-stage"):
        tspws.Plan(two, N).weighted_stack_batch(X, [0, 5, 9], w)
    with pytest.raises(tspws.TspwsError, match="weight"):
        pl.weighted_stack_batch(X, [0, 6, 9], bad_weight(-0.5))
    assert cabi(k=None) == 0  # (the arguments above are fine when nothing is wrong with them; Keff is optional)
    torch.cuda.synchronize()
    assert (sm == [[6] * M, [3] * M]).all() and not (rep != 0).any().item() and (ke == 7.5).all()  # (zero traces: zero stacks)
    assert cabi() == 0 and (ke == [[6.0] * M, [3.0] * M]).all()
    st = pl.weighted_stack_batch_stats()
    assert st == dict(shared=2, empty=0, rounds=1, rows=2 * M), st
    # the binding's own checks
    f = [0, 6, 9]
    call = pl.weighted_stack_batch
    bad = [
        lambda: call(X.double(), f, w),                                          # traces not float32
        lambda: call(X, f, w.astype(np.float32)),                                # weights not float64
        lambda: call(X, f, w[:, :-1]),                                           # weights of another width
        lambda: call(X, f, w[0]),                                                # weights not 2-D
        lambda: call(X, [0, 6, 5], w),                                           # decreasing offsets
        lambda: call(X, [0, 6, 10], w),                                          # past the rows
        lambda: call(X, f, w, ls_out=torch.zeros((2, M, N + 1), device="cuda")),
        lambda: call(X, f, w, ts_out=torch.zeros((2, M, N), dtype=torch.float64, device="cuda")),
        lambda: call(X, f, w, mtr_out=np.zeros((2, M), np.int32)),
        lambda: call(X, f, w, mtr_out=np.zeros((M, 2), np.uint32)),
    ]
    for k, bf in enumerate(bad):
        with pytest.raises(tspws.TspwsError):
            bf()
            pytest.fail(f"bad argument {k} accepted")
    sl, st2, m, keff = call(X, [4], np.ones((M, 0), np.float64))
    assert tuple(sl.shape) == (0, M, N) and m.shape == (0, M) and keff.shape == (0, M)
