"""CPU-side checks of the percentile bands over replica rows (tspws_hip_replica_bands): the library exports the entry points and the binding
declares them; every refusal that needs no device, with a NULL plan, host dummies and sentinel-filled outputs unchanged; and the checker's
own test -- tests/replica_bands_ref.py against np.quantile(method="linear") in FP64, within 1 float32 ulp (numpy interpolates with a
different but equivalent expression above g = 0.5, so 1 ulp is the condition, not 0)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import replica_bands_ref as rbr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_replica_bands", "tspws_hip_replica_bands_stats")
QS = [0, 0.025, 0.16, 1 / 3, 0.5, 0.84, 0.975, 1]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, rows=True, q=(0.025, 0.5, 0.975), Q=None, bands=True, qptr=True, B=2, M=3, ld=256, mtr=False):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    dummy = np.full(16, 7.0, np.float32)
    out = np.full(16, -3.0, np.float32)
    qa = np.array(q, dtype=np.float64)
    m = np.ones(max(1, B * M), np.uint32)
    rc = lib.tspws_hip_replica_bands(None, dummy.ctypes.data if rows else None, ld, B, M, m.ctypes.data if mtr else None, qa.ctypes.data if qptr else None,
                                     qa.size if Q is None else Q, out.ctypes.data if bands else None, None)
    assert (out == -3.0).all() and (dummy == 7.0).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("replica_bands", "replica_bands_stats"):
        assert hasattr(tspws.Plan, n), n
    stats = (C.c_uint * 5)()
    assert lib.tspws_hip_replica_bands_stats(None, C.byref(stats)) == -1
    assert b"replica_bands_stats: NULL" in lib.tspws_hip_last_error()


def test_null_arguments(lib):
    for kw in (dict(), dict(mtr=True), dict(rows=False), dict(qptr=False), dict(bands=False)):  # (the first two: the NULL plan)
        rc, err = call(lib, **kw)
        assert rc == -1 and b"replica_bands: NULL" in err, (kw, err)
    # B == 0 / M == 0 / Q == 0 do nothing, but a NULL plan is still an error (as in the other batch calls; tests/test_replica_bands_gpu.py
    # has them with a plan: they return 0)
    for kw in (dict(B=0), dict(M=0), dict(Q=0)):
        rc, err = call(lib, **kw)
        assert rc == -1 and b"replica_bands: NULL" in err, (kw, err)
    # a short row stride needs the plan's trace length, so that the NULL plan is what refuses it here
    rc, err = call(lib, ld=3)
    assert rc == -1 and b"replica_bands: NULL" in err, err


def test_refused_quantiles(lib):
    rc, err = call(lib, q=[0.1] * 9)
    assert rc == -1 and b"replica_bands: more than 8" in err, err
    for bad in (float("nan"), -1e-9, 1.0000001, float("inf"), -float("inf")):
        rc, err = call(lib, q=[0.5, bad])
        assert rc == -1 and b"replica_bands: a probability outside" in err, (bad, err)
    # what needs no plan comes first: these are not the NULL plan's message
    for ok in ([0.0], [1.0], [0.0, 1.0, 0.5]):
        rc, err = call(lib, q=ok)
        assert rc == -1 and b"replica_bands: NULL" in err, (ok, err)


# ---- the checker's own test ------------------------------------------------------------------------------------------------------------------
def checker_rows(M, seed):
    """[M][193] float32: columns of widely different scale, a constant column, a column of integers (ties), a column of mixed -0.0 / +0.0."""
    rng = np.random.default_rng(seed)
    N = 193
    x = rng.standard_normal((M, N)).astype(np.float32) * (10.0 ** rng.uniform(-6, 2, N)).astype(np.float32)
    x[:, 1] = -7.25
    x[:, 2] = rng.integers(-3, 4, M).astype(np.float32)
    x[:, 4] = np.where(rng.integers(0, 2, M) == 1, np.float32(-0.0), np.float32(0.0))
    return x


def test_checker_against_numpy_quantile():
    exact = total = 0
    worst = 0.0
    for M in (1, 2, 9, 100, 101, 700):
        rows = checker_rows(M, seed=100 + M)
        got = rbr.expected(rows[None], QS)[0]
        want = np.quantile(rows.astype(np.float64), QS, axis=0, method="linear").astype(np.float32)
        assert got.shape == want.shape == (len(QS), rows.shape[1])
        ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)
        ulp = np.where(got == want, 0.0, ulp)
        exact += int((got == want).sum())
        total += got.size
        worst = max(worst, float(ulp.max()))
        assert (ulp <= 1.0).all(), (M, float(ulp.max()))
        # q = 0 / 1 are the extremes, the bands do not decrease in q
        assert np.array_equal(got[0], rows.min(axis=0)) and np.array_equal(got[-1], rows.max(axis=0))
        assert (np.diff(got, axis=0) >= 0).all()
    print(f"checker vs np.quantile: {exact} of {total} values exact, worst {worst:.2f} ulp")


def test_checker_counts():
    """Replicas with a count of 0 do not take part; none gives zero bands, one gives that row for every q."""
    rows = np.stack([checker_rows(9, seed=5), checker_rows(9, seed=6), checker_rows(9, seed=7)])
    mtr = np.array([[4, 0, 1, 9, 0, 2, 2, 0, 1], [0] * 9, [0, 0, 0, 0, 0, 6, 0, 0, 0]], np.uint32)
    got = rbr.expected(rows, QS, mtr)
    np.testing.assert_array_equal(got[0], rbr.expected(rows[:1, mtr[0] > 0], QS)[0])
    assert not got[1].any()
    for k in range(len(QS)):
        np.testing.assert_array_equal(got[2, k], rows[2, 5])
