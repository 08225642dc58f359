"""CPU-side checks of the real-weighted stacks (tspws_hip_weighted_stack_batch, tspws_weights_from_scores): the library exports the entry
points and the binding declares them; every refusal that needs no device, with sentinel-filled outputs unchanged; the host weight rule
against a numpy restatement; and the checker's own tests -- tests/weighted_batch_ref.py against tests/boot_batch_ref.py (itself proved equal
to the oracle's subsampling by tests/test_bootstrap_batch_cpu.py) on 0/1 rows (bit for bit) and on integer rows in the biased modes, its
invariance under a power-of-two scaling, and Keff of an all-equal row."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import abi
import boot_batch_ref as bbr
import weighted_batch_ref as wbr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_weighted_stack_batch", "tspws_hip_weighted_stack_batch_stats", "tspws_weights_from_scores")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, p=True, first=(0, 6, 9), w=True, Mn=3, ls_out=True, ts_out=True, mtr_out=True, keff=True, ld=256, x=True, B=None, Kmax=10, weights=None):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64) if first is not None else None
    B = (f.size - 1 if f is not None else 2) if B is None else B
    wm = np.ones((max(Mn, 1), 9), np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    pp = abi.default_params(Kmax=Kmax)
    dummy = np.full(16, 7.0, np.float32)
    m = np.full(max(1, B * Mn), 99, np.uint32)
    ke = np.full(max(1, B * Mn), 7.5, np.float64)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_weighted_stack_batch(None, C.byref(pp) if p else None, ptr(x, dummy), ld, ptr(f is not None, f) if f is not None else None, B, Mn, ptr(w, wm),
                                            ptr(ls_out, dummy), ptr(ts_out, dummy), ptr(mtr_out, m), ptr(keff, ke), None)
    assert (m == 99).all() and (dummy == 7.0).all() and (ke == 7.5).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("weighted_stack_batch", "weighted_stack_batch_stats"):
        assert hasattr(tspws.Plan, n), n
    assert hasattr(tspws, "weights_from_scores")
    stats = (C.c_uint * 4)()
    assert lib.tspws_hip_weighted_stack_batch_stats(None, C.byref(stats)) == -1
    assert b"weighted_stack_batch_stats: NULL" in lib.tspws_hip_last_error()


def test_null_arguments(lib):
    for kw in (dict(p=False), dict(first=None), dict(ls_out=False), dict(ts_out=False), dict(mtr_out=False), dict(w=False), dict(), dict(keff=False)):  # (the last two: NULL plan)
        rc, err = call(lib, **kw)
        assert rc == -1 and b"weighted_stack_batch: NULL" in err, (kw, err)
    # B == 0 / M == 0 do nothing, but a NULL plan is still an error (tests/test_weighted_stack_batch_gpu.py has them with a plan: they return 0)
    for kw in (dict(B=0), dict(Mn=0), dict(B=0, p=False), dict(Mn=0, p=False)):
        rc, err = call(lib, **kw)
        assert rc == -1 and b"weighted_stack_batch: NULL" in err, (kw, err)


def test_inconsistent_arguments(lib):
    rc, err = call(lib, first=(0, 8, 6))
    assert rc == -1 and b"weighted_stack_batch: decreasing" in err, err
    # a two-stage ensemble needs no plan to be seen: Kmax = 2 <= 5 traces; so does one beside an empty and a single-stage ensemble
    for first in ((0, 5), (0, 0, 1, 9)):
        rc, err = call(lib, first=first, Kmax=2)
        assert rc == -1 and b"weighted_stack_batch: " in err and b"two-stage" in err, err
    # ... while Kmax above every ensemble (or 0) is single-stage: only the NULL plan refuses
    for kmax in (0, 7):
        rc, err = call(lib, Kmax=kmax)
        assert rc == -1 and b"weighted_stack_batch: NULL" in err, err
    # NULL traces and a short row stride need the plan's trace length, so that the NULL plan is what refuses them here
    for kw in (dict(x=False), dict(ld=3)):
        rc, err = call(lib, **kw)
        assert rc == -1 and b"weighted_stack_batch: NULL" in err, (kw, err)


@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf"), -float("inf"), -1e-300])
def test_bad_weights(lib, bad):
    for r, c in ((0, 0), (2, 8), (1, 5)):
        w = np.ones((3, 9))
        w[r, c] = bad
        rc, err = call(lib, weights=w)
        assert rc == -1 and b"weighted_stack_batch: " in err and b"weight" in err, err


def test_row_sums_not_finite(lib):
    w = np.ones((3, 9))
    w[1, :6] = 1e308   # W overflows
    rc, err = call(lib, weights=w)
    assert rc == -1 and b"weighted_stack_batch: " in err and b"not finite" in err, err
    w = np.ones((3, 9))
    w[2, 7] = 1e200    # W is finite, Q overflows
    rc, err = call(lib, weights=w)
    assert rc == -1 and b"weighted_stack_batch: " in err and b"not finite" in err, err
    w = np.ones((3, 9))
    w[0, :6] = [0, 1e-200, 0, 0, 1e-190, 0]  # Q underflows to zero: Keff would be 0 / 0
    rc, err = call(lib, weights=w)
    assert rc == -1 and b"weighted_stack_batch: " in err and b"underflow" in err, err


# ---- the host weight rule ---------------------------------------------------------------------------------------------------------------------
def weights_numpy(score, first, rule, a):
    """tspws_weights_from_scores restated (libm's pow element by element)."""
    w = np.zeros(len(score))
    for b in range(len(first) - 1):
        c0, c1 = first[b] - first[0], first[b + 1] - first[0]
        s = score[c0:c1]
        if rule == 0:
            w[c0:c1] = [math.pow(v, a) if v > 0 else 0.0 for v in s]
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.where((s > 0) & np.isfinite(s), 1.0 / s, 0.0)
            w[c0:c1] = v / v.max() if len(v) and v.max() > 0 else 0.0
    return w


def test_weights_from_scores(lib):
    nan, inf = float("nan"), float("inf")
    first = [3, 8, 8, 11, 14, 15]
    rng = np.random.default_rng(3)
    score = np.concatenate([rng.uniform(0.05, 1.0, 5), [nan, inf, -0.5], [nan, -1.0, 0.0], [2.5e-7]])
    score[1], score[3] = nan, -0.25
    assert len(score) == first[-1] - first[0]
    for rule, name, a in ((0, "power", 2.0), (0, "power", 0.5), (0, "power", 1.0), (1, "inverse", 0.0), (1, "inverse", nan)):
        want = weights_numpy(score, first, rule, a)
        for r in (rule, name):
            got = tspws.weights_from_scores(score, first, r, a)
            assert got.dtype == np.float64 and np.array_equal(got, want), (rule, a, got, want)
    # rule 0: NaN and non-positive scores give 0, an infinite score its power
    w = tspws.weights_from_scores(score, first, 0, 2.0)
    assert w[1] == 0 and w[3] == 0 and w[5] == 0 and w[6] == inf and w[7] == 0 and not w[8:11].any() and w[0] == score[0] * score[0]
    # rule 1: the ensemble's best trace has weight 1, dead scores 0, an ensemble without a positive finite score zeros
    w = tspws.weights_from_scores(score, first, 1, 0.0)
    assert w[:5].max() == 1.0 and w[1] == 0 and w[3] == 0 and not w[5:8].any() and not w[8:11].any() and w[11] == 1.0
    assert (w >= 0).all() and np.isfinite(w).all()
    # the return codes of the C entry
    f = np.array(first, dtype=np.uint64)
    out = np.full(len(score), 7.0)
    fn = lib.tspws_weights_from_scores
    assert fn(None, score.ctypes.data, f.ctypes.data, 5, 0, 1.0) == 1 and fn(out.ctypes.data, None, f.ctypes.data, 5, 0, 1.0) == 1
    assert fn(out.ctypes.data, score.ctypes.data, None, 5, 0, 1.0) == 1
    dec = np.array([0, 5, 4], dtype=np.uint64)
    assert fn(out.ctypes.data, score.ctypes.data, dec.ctypes.data, 2, 0, 1.0) == 1
    assert fn(out.ctypes.data, score.ctypes.data, f.ctypes.data, 5, 2, 1.0) == 2 and fn(out.ctypes.data, score.ctypes.data, f.ctypes.data, 5, -1, 1.0) == 2
    assert fn(out.ctypes.data, score.ctypes.data, f.ctypes.data, 5, 0, nan) == 2
    assert (out == 7.0).all()  # nothing written by a refused call
    assert fn(out.ctypes.data, score.ctypes.data, f.ctypes.data, 5, 1, nan) == 0 and np.array_equal(out, w)
    with pytest.raises(tspws.TspwsError):
        tspws.weights_from_scores(score, first, "median", 1.0)
    with pytest.raises(tspws.TspwsError):
        tspws.weights_from_scores(score[:-1], first, 0, 1.0)
    with pytest.raises(tspws.TspwsError):
        tspws.weights_from_scores(score, first, 0, nan)


# ---- the checker's own tests -------------------------------------------------------------------------------------------------------------------
N, MTR = 256, 7
KW = [dict(), dict(unbiased=1), dict(wu=1.0), dict(wu=1.5, type=-3)]
IDS = ["biased", "unbiased", "wu1", "wu1.5-mexhat"]
ROWS = np.array([[0, 3, 1, 0, 2, 1, 0], [5, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1], [1, 0, 1, 1, 0, 0, 1]], np.uint8)
_X = abi.synth_traces(MTR + 2, N, seed=9)
FIRST = [2, 2 + MTR]


@pytest.mark.parametrize("kw", KW, ids=IDS)
def test_checker_on_masks_is_the_bootstrap_checker(kw):
    """0/1 rows: bit for bit the rows of tests/boot_batch_ref.py on the same rows as counts -- W = Keff = K, a product by 1 is no operation."""
    p = abi.resolve(abi.default_params(**kw), N)
    sel = ROWS[[2, 3, 4, 5]]
    ls, ts, K, keff = wbr.expected(p, _X, FIRST, sel.astype(np.float64))
    wl, wt, wk = bbr.expected(p, _X, FIRST, sel)
    np.testing.assert_array_equal(K, wk)
    np.testing.assert_array_equal(keff, wk.astype(np.float64))
    assert (np.abs(wt[0, [0, 2, 3]]).max(axis=1) > 0).all() and not wt[0, 1].any()
    np.testing.assert_array_equal(ls, wl)
    np.testing.assert_array_equal(ts, wt)


@pytest.mark.parametrize("kw", [KW[0], KW[2], KW[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_checker_on_counts_agrees_with_the_bootstrap_checker(kw):
    """Integer rows in the biased modes: within 2e-6 of tests/boot_batch_ref.py on the same counts (the float accumulator multiplies once where
    that one adds repeatedly; W = sum c = its K).  The UNBIASED mode is deliberately not compared: the weighted estimator removes the bias
    1 / Keff with Keff = (sum c)^2 / sum c^2, the effective number of independent traces, while the bootstrap's expanded ensemble removes
    1 / K with K = sum c, counting every copy as a trace of its own -- two different estimators wherever a count exceeds 1."""
    p = abi.resolve(abi.default_params(**kw), N)
    ls, ts, K, keff = wbr.expected(p, _X, FIRST, ROWS.astype(np.float64))
    wl, wt, wk = bbr.expected(p, _X, FIRST, ROWS)
    np.testing.assert_array_equal(K[0], (ROWS > 0).sum(axis=1))
    worst = 0.0
    for m in range(len(ROWS)):
        if not wk[0, m]:
            assert not ls[0, m].any() and not ts[0, m].any() and keff[0, m] == 0
            continue
        c = ROWS[m].astype(np.float64)
        assert keff[0, m] == c.sum() ** 2 / (c * c).sum()
        worst = max(worst, abi.relerr(ls[0, m], wl[0, m]), abi.relerr(ts[0, m], wt[0, m]))
    print("integer rows against the bootstrap checker: worst relerr", worst)
    assert worst <= 2e-6


@pytest.mark.parametrize("kw", KW, ids=IDS)
def test_checker_power_of_two_scaling(kw):
    """w and 0.25 w give the same bits: every product, sum and quotient of the definition scales exactly."""
    p = abi.resolve(abi.default_params(**kw), N)
    w = np.random.default_rng(5).uniform(0.01, 3.0, (4, MTR))
    w[1, [0, 3]] = 0
    w[2] = 0
    w[2, 4] = 1.7
    a = wbr.expected(p, _X, FIRST, w)
    b = wbr.expected(p, _X, FIRST, 0.25 * w)
    assert (np.abs(a[1][0]).max(axis=1) > 0).all()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[2][0].tolist() == [MTR, MTR - 2, 1, MTR] and a[3][0, 2] == 1.0 and (a[3][0] <= a[2][0]).all()


def test_checker_keff_of_equal_weights():
    """Keff of n equal weights is n: W and Q take n - 1 rounded additions each, Q n rounded squares, then a product and a quotient -- at most
    3 n + 3 roundings of 2^-53 relative, each entering W W / Q once or twice."""
    for v in (1.0, 0.25, 3.0, 1e-6, 1e6):
        for n in (1, 2, 7, 64):
            npos, W, Q, keff = wbr.row_sums(np.concatenate([np.full(n, v), [0.0, 0.0]]))
            assert npos == n and abs(keff - n) <= (3 * n + 3) * 2.0 ** -53 * n, (v, n, keff)
    for v in (1.0, 0.25, 4.0):  # powers of two: exactly
        assert wbr.row_sums(np.full(7, v))[3] == 7.0
    assert wbr.row_sums(np.zeros(5)) == (0, 0.0, 0.0, 0.0)
