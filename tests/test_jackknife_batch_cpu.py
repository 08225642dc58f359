"""CPU-side checks of the batched single-stage jackknife (tspws_hip_jackknife_batch): the library refuses bad arguments before any device
work (every check that needs no plan comes before the plan is looked at, so a host without a GPU sees each of them), the binding declares
the entry points, and jackknife_selection_batch builds every ensemble's columns like the oracle's JackknifePlans restatement."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import abi
import jk_single_ref as ref

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, plan=None, p=True, first=(0, 4, 8), sel=True, Cn=3, main=(True, True), ls_out=True, ts_out=True, mtr_out=True, ld=256, params=None,
         sel_array=None):
    """One call with host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64)
    B = f.size - 1
    T = int(f[-1] - f[0]) if (np.diff(f.astype(np.int64)) >= 0).all() else 8
    s = np.ones((Cn, max(T, 1)), np.int8) if sel_array is None else sel_array
    pp = params if params is not None else abi.default_params()
    dummy = np.zeros(16, np.float32)
    m = np.zeros(max(B * Cn, 1), np.uint32)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_jackknife_batch(plan, C.byref(pp) if p else None, dummy.ctypes.data, ld, f.ctypes.data if first is not None else None, B,
                                       ptr(sel, s), Cn, ptr(main[0], dummy), ptr(main[1], dummy), ptr(ls_out, dummy), ptr(ts_out, dummy),
                                       ptr(mtr_out, m), None)
    return rc, lib.tspws_hip_last_error()


def test_null_arguments(lib):
    for kw in (dict(p=False), dict(sel=False), dict(ls_out=False), dict(ts_out=False), dict(mtr_out=False), dict()):  # (the last: NULL plan)
        rc, err = call(lib, **kw)
        assert rc == -1 and b"jackknife_batch: NULL" in err, (kw, err)
    p = abi.default_params()
    assert lib.tspws_hip_jackknife_batch(None, C.byref(p), None, 256, None, 2, None, 3, None, None, None, None, None, None) == -1
    assert b"NULL" in lib.tspws_hip_last_error()
    stats = (C.c_uint * 6)()
    assert lib.tspws_hip_jackknife_batch_stats(None, C.byref(stats)) == -1


def test_inconsistent_arguments(lib):
    for main in ((True, False), (False, True)):
        rc, err = call(lib, main=main)
        assert rc == -1 and b"exactly one" in err, err
    rc, err = call(lib, first=(0, 6, 4))
    assert rc == -1 and b"decreasing" in err, err
    # a two-stage parameter set for one ensemble (Kmax = 4 <= 4 traces)
    rc, err = call(lib, params=abi.default_params(Kmax=4))
    assert rc == -1 and b"two-stage" in err, err
    rc, err = call(lib, params=abi.default_params(Kmax=5))  # (Kmax > M_b everywhere: single-stage, so the NULL plan is what refuses)
    assert rc == -1 and b"jackknife_batch: NULL" in err, err
    # more than 65535 distinct selection columns in one ensemble: 17 rows that spell the column's number in binary
    T = 65536 + 40
    cols = np.arange(T, dtype=np.uint32) % 65537
    big = ((cols[None, :] >> np.arange(17, dtype=np.uint32)[:, None]) & 1).astype(np.int8)
    rc, err = call(lib, first=(0, 30, T), Cn=17, sel_array=np.ascontiguousarray(big))
    assert rc == -1 and b"65535" in err, err


def test_binding_declares_the_entry_points(lib):
    assert "tspws_hip_jackknife_batch" in tspws.SYMBOLS and "tspws_hip_jackknife_batch_stats" in tspws.SYMBOLS
    assert hasattr(tspws.Plan, "jackknife_batch") and hasattr(tspws.Plan, "jackknife_batch_stats")
    assert callable(tspws.jackknife_selection_batch)


@pytest.mark.parametrize("n,d", [(4, 1), (5, 2), (12, 1)])
def test_selection_helper_matches_the_oracle(lib, n, d):
    sizes = [40, 1, 0, 130, 7]
    first = np.concatenate([[3], 3 + np.cumsum(sizes)]).astype(np.int64)
    times = np.zeros(int(first[-1]), np.int64)
    for b, m in enumerate(sizes):
        if m:
            times[first[b]:first[b + 1]] = ref.leap_times(m, seed=10 + b) if m > 1 else ref.leap_times(2, seed=1)[-1:]  # (31 Dec of a leap year: bin n)
    sel = tspws.jackknife_selection_batch(times, first, n, d)
    assert sel.dtype == np.int8 and sel.shape == (abi.binomial(n, d), sum(sizes))
    never_deleted = 0
    for b, m in enumerate(sizes):
        blk = sel[:, first[b] - 3:first[b + 1] - 3]
        if m:
            np.testing.assert_array_equal(blk, ref.selection(times[first[b]:first[b + 1]], n, d))
            never_deleted += int(blk.all(axis=0).sum())
    assert never_deleted >= 3  # the never-deleted bin n occurs (leap_times)
    bad = times.copy()
    bad[first[3]] = 0
    with pytest.raises(tspws.TspwsError):
        tspws.jackknife_selection_batch(bad, first, n, d)
    with pytest.raises(tspws.TspwsError):
        tspws.jackknife_selection_batch(times, [0, 5, 3], n, d)


# ---- the module-level helpers' check of `first` -------------------------------------------------------------------------------------------
# one good `first` (offset start, an empty ensemble) and one plane of scores; the expected arrays were recorded from the binding as it was
# before its helpers shared one check of `first` (abi.srand(5) before the two drawing helpers)
FIRST = [3, 3, 7]
TIMES = 1_000_000_000 + 86400 * 40 * np.arange(7)
SCORE = np.array([0.9, float("nan"), 0.2, 0.85])
HELPERS = {
    "jackknife_selection_batch": lambda f: tspws.jackknife_selection_batch(TIMES, f, 4, 1),
    "subsampling_selection_batch": lambda f: tspws.subsampling_selection_batch(f, 3, 0.5),
    "bootstrap_counts_batch": lambda f: tspws.bootstrap_counts_batch(f, 3),
    "selection_from_scores": lambda f: tspws.selection_from_scores(SCORE, f, "threshold", 0.5),
    "weights_from_scores": lambda f: tspws.weights_from_scores(SCORE, f, "power", 2.0),
}
BAD_FIRST = {"2-D": [[0, 1], [2, 3]], "float": [0.0, 1.0], "negative": [-1, 2], "decreasing": [0, 5, 4], "empty": []}


@pytest.mark.parametrize("bad", sorted(BAD_FIRST))
@pytest.mark.parametrize("helper", sorted(HELPERS))
def test_helpers_refuse_a_bad_first(lib, helper, bad):
    with pytest.raises(tspws.TspwsError):
        HELPERS[helper](BAD_FIRST[bad])


@pytest.mark.parametrize("as_array", [list, lambda f: np.array(f, np.int32), lambda f: np.array(f, np.uint64)])
def test_helpers_on_a_good_first(lib, as_array):
    f = as_array(FIRST)
    jk = HELPERS["jackknife_selection_batch"](f)
    assert jk.dtype == np.int8 and jk.tolist() == [[0, 0, 0, 1], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1]]
    abi.srand(5)
    sub = HELPERS["subsampling_selection_batch"](f)
    assert sub.dtype == np.int8 and sub.tolist() == [[1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 1]]
    abi.srand(5)
    cnt = HELPERS["bootstrap_counts_batch"](f)
    assert cnt.dtype == np.uint8 and cnt.tolist() == [[2, 1, 0, 1], [2, 2, 0, 0], [1, 2, 0, 1]]
    sel, kept = HELPERS["selection_from_scores"](f)
    assert (sel.dtype, sel.tolist(), kept.dtype, kept.tolist()) == (np.int8, [1, 0, 0, 1], np.uint32, [0, 2])
    sel, kept = tspws.selection_from_scores(SCORE, f, "mad", 1.0)
    assert (sel.tolist(), kept.tolist()) == ([1, 0, 0, 1], [0, 2])
    w = HELPERS["weights_from_scores"](f)
    assert w.dtype == np.float64 and [x.hex() for x in w] == ["0x1.9eb851eb851ecp-1", "0x0.0p+0", "0x1.47ae147ae147cp-5", "0x1.71eb851eb851ep-1"]
    w = tspws.weights_from_scores(SCORE, f, "inverse")
    assert [x.hex() for x in w] == ["0x1.c71c71c71c71dp-3", "0x0.0p+0", "0x1.0000000000000p+0", "0x1.e1e1e1e1e1e1ep-3"]
