"""CPU-side checks of the batched random subsampling (tspws_hip_subsample_batch / _sel, tspws_subsampling_plan_batch): the library exports
the entry points and the binding declares them; the host mask helper draws in the rand() order of a loop of single calls over the ensembles;
and every refusal comes before the plan is looked at or right behind it, so a host without a GPU sees each of them with outputs untouched."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import abi

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_subsampling_plan_batch", "tspws_hip_subsample_batch_sel", "tspws_hip_subsample_batch", "tspws_hip_subsample_batch_stats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, drawing=False, p=True, first=(0, 12, 24), sel=True, Mn=3, ls_out=True, ts_out=True, mtr_out=True, ld=256, x=True, B=None):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64) if first is not None else None
    B = (f.size - 1 if f is not None else 2) if B is None else B
    s = np.ones((Mn, 24), np.int8)
    pp = abi.default_params(Kmax=10, subsmpl_p=0.5)
    dummy = np.zeros(16, np.float32)
    m = np.full(max(1, B * Mn), 99, np.uint32)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    head = (None, C.byref(pp) if p else None, ptr(x, dummy), ld, ptr(f is not None, f) if f is not None else None, B, Mn)
    tail = (ptr(ls_out, dummy), ptr(ts_out, dummy), ptr(mtr_out, m), None)
    abi.srand(11)
    r0 = C.CDLL(None).rand()
    abi.srand(11)
    if drawing:
        rc = lib.tspws_hip_subsample_batch(*head, *tail)
    else:
        rc = lib.tspws_hip_subsample_batch_sel(*head, ptr(sel, s), *tail)
    assert (m == 99).all() and not dummy.any()  # outputs untouched
    assert C.CDLL(None).rand() == r0              # ... and a refused call draws nothing
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("subsample_batch", "subsample_batch_stats", "subsample_sel"):
        assert hasattr(tspws.Plan, n), n
    assert hasattr(tspws, "subsampling_selection_batch")
    stats = (C.c_uint * 6)()
    assert lib.tspws_hip_subsample_batch_stats(None, C.byref(stats)) == -1
    assert b"subsample_batch_stats: NULL" in lib.tspws_hip_last_error()


SIZES = [0, 1, 5, 64, 0, 30]


@pytest.mark.parametrize("prob", [0.2, 0.5, 0.8, 1.0])
def test_plan_batch_draws_like_a_loop_of_single_calls(lib, prob):
    orc = abi.oracle()
    M, first0 = 3, 4
    first = np.concatenate([[first0], first0 + np.cumsum(SIZES)]).astype(np.uint64)
    T = int(first[-1] - first[0])
    for seed in (1, 77):
        got = np.full((M, T), 7, np.int8)
        abi.srand(seed)
        assert lib.tspws_subsampling_plan_batch(got.ctypes.data, first.ctypes.data, len(SIZES), M, prob) == 0
        after = C.CDLL(None).rand()
        want = np.full((M, T), 7, np.int8)
        abi.srand(seed)
        for b, mb in enumerate(SIZES):
            K = math.ceil(mb * prob)
            for m in range(M):
                if not mb:
                    continue
                row = np.zeros(mb, np.int8)
                assert orc.orc_subsampling_plan(row.ctypes.data, mb, K) == 0
                c0 = int(first[b] - first[0])
                want[m, c0:c0 + mb] = row
        assert C.CDLL(None).rand() == after  # the same number of draws
        np.testing.assert_array_equal(got, want)  # byte for byte
        for b, mb in enumerate(SIZES):
            c0 = int(first[b] - first[0])
            assert ((got[:, c0:c0 + mb] == 1).sum(axis=1) == math.ceil(mb * prob)).all(), (b, prob)
            assert np.isin(got[:, c0:c0 + mb], (0, 1)).all()
        # the binding draws through the same function
        abi.srand(seed)
        np.testing.assert_array_equal(tspws.subsampling_selection_batch(first, M, prob), want)


def test_plan_batch_refusals(lib):
    first = np.array([0, 5, 9], dtype=np.uint64)
    sel = np.full((2, 9), 7, np.int8)
    abi.srand(3)
    r0 = C.CDLL(None).rand()
    abi.srand(3)
    assert lib.tspws_subsampling_plan_batch(None, first.ctypes.data, 2, 2, 0.5) == 1
    assert lib.tspws_subsampling_plan_batch(sel.ctypes.data, None, 2, 2, 0.5) == 1
    bad = np.array([0, 5, 4], dtype=np.uint64)
    assert lib.tspws_subsampling_plan_batch(sel.ctypes.data, bad.ctypes.data, 2, 2, 0.5) == 1
    assert (sel == 7).all() and C.CDLL(None).rand() == r0
    with pytest.raises(tspws.TspwsError):
        tspws.subsampling_selection_batch([0, 5, 4], 2, 0.5)
    with pytest.raises(tspws.TspwsError):
        tspws.subsampling_selection_batch([0, 5, 9], 2, 1.5)
    assert tspws.subsampling_selection_batch([3, 3], 2, 0.5).shape == (2, 0)


@pytest.mark.parametrize("drawing", [False, True])
def test_null_arguments(lib, drawing):
    cases = [dict(p=False), dict(first=None), dict(ls_out=False), dict(ts_out=False), dict(mtr_out=False), dict()]  # (the last: NULL plan)
    if not drawing:
        cases.append(dict(sel=False))
    for kw in cases:
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"subsample_batch: NULL" in err, (kw, err)
    # B == 0 / M == 0 do nothing, but a NULL plan is still an error
    for kw in (dict(B=0), dict(Mn=0)):
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"subsample_batch: NULL" in err, (kw, err)


@pytest.mark.parametrize("drawing", [False, True])
def test_inconsistent_arguments(lib, drawing):
    rc, err = call(lib, drawing=drawing, first=(0, 16, 12))
    assert rc == -1 and b"subsample_batch: decreasing" in err, err
    # decreasing offsets are seen before the NULL plan; NULL traces and a short row stride need the plan's trace length, so that the NULL
    # plan is what refuses them here (tests/test_subsample_batch_gpu.py has them with a plan)
    for kw in (dict(x=False), dict(ld=3)):
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"subsample_batch: NULL" in err, (kw, err)
    # mixed kinds are no refusal: with Kmax = 10 the ensembles of 6 and 18 traces are single- and two-stage, and only the NULL plan refuses
    rc, err = call(lib, drawing=drawing, first=(0, 6, 24))
    assert rc == -1 and b"subsample_batch: NULL" in err, err
