"""CPU-side checks of the batched two-stage jackknife (tspws_hip_jackknife_batch_two_stage): the library exports the entry points, the
binding declares them, and the refusals that need no plan come before the plan is looked at, so a host without a GPU sees each of them."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import abi

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, p=True, first=(0, 12, 24), sel=True, Cn=3, main=(True, True), ls_out=True, ts_out=True, mtr_out=True, ld=256, params=None):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64)
    B = f.size - 1
    s = np.ones((Cn, 24), np.int8)
    pp = params if params is not None else abi.default_params(Kmax=10)
    dummy = np.zeros(16, np.float32)
    m = np.full(B * Cn, 99, np.uint32)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_jackknife_batch_two_stage(None, C.byref(pp) if p else None, dummy.ctypes.data, ld, f.ctypes.data if first is not None else None,
                                                 B, ptr(sel, s), Cn, ptr(main[0], dummy), ptr(main[1], dummy), ptr(ls_out, dummy), ptr(ts_out, dummy),
                                                 ptr(mtr_out, m), None)
    assert (m == 99).all() and not dummy.any()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    assert hasattr(lib, "tspws_hip_jackknife_batch_two_stage") and hasattr(lib, "tspws_hip_jackknife_batch_two_stage_stats")
    assert "tspws_hip_jackknife_batch_two_stage" in tspws.SYMBOLS and "tspws_hip_jackknife_batch_two_stage_stats" in tspws.SYMBOLS
    assert hasattr(tspws.Plan, "jackknife_batch_two_stage") and hasattr(tspws.Plan, "jackknife_batch_two_stage_stats")
    stats = (C.c_uint * 6)()
    assert lib.tspws_hip_jackknife_batch_two_stage_stats(None, C.byref(stats)) == -1


def test_null_arguments(lib):
    for kw in (dict(p=False), dict(first=None), dict(sel=False), dict(ls_out=False), dict(ts_out=False), dict(mtr_out=False), dict()):  # (the last: NULL plan)
        if kw.get("first", 0) is None:
            p = abi.default_params(Kmax=10)
            rc = lib.tspws_hip_jackknife_batch_two_stage(None, C.byref(p), None, 256, None, 2, None, 3, None, None, None, None, None, None)
            err = lib.tspws_hip_last_error()
        else:
            rc, err = call(lib, **kw)
        assert rc == -1 and b"jackknife_batch_two_stage: NULL" in err, (kw, err)
    # B == 0 / C == 0 do nothing, but a NULL plan is still an error
    p = abi.default_params(Kmax=10)
    f = np.array([0, 12, 24], dtype=np.uint64)
    assert lib.tspws_hip_jackknife_batch_two_stage(None, C.byref(p), None, 256, f.ctypes.data, 0, None, 3, None, None, None, None, None, None) == -1


def test_inconsistent_arguments(lib):
    for main in ((True, False), (False, True)):
        rc, err = call(lib, main=main)
        assert rc == -1 and b"exactly one" in err, err
    rc, err = call(lib, first=(0, 16, 12))
    assert rc == -1 and b"decreasing" in err, err
    # an ensemble that is single-stage: Kmax = 10 > 6 traces, or no two-stage rule at all
    rc, err = call(lib, first=(0, 18, 24))
    assert rc == -1 and b"single-stage" in err, err
    rc, err = call(lib, params=abi.default_params())
    assert rc == -1 and b"single-stage" in err, err
    # an empty ensemble is no single-stage ensemble: the NULL plan is what refuses
    rc, err = call(lib, first=(0, 24, 24))
    assert rc == -1 and b"jackknife_batch_two_stage: NULL" in err, err
