"""CPU-side checks of the batched convergence curves (tspws_hip_convergence_batch): the library exports the entry points, the binding
declares them, and the refusals that need no plan come before the plan is looked at, so a host without a GPU sees each of them."""
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


def call(lib, p=True, first=(0, 12, 24), traces=True, ref_ts=True, ref_ls=True, curves=(True, True, True, True), ld=256):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64)
    B = f.size - 1
    pp = abi.default_params(Kmax=10)
    dummy = np.zeros(16, np.float32)
    cur = [np.full(24, 99.0) for _ in range(4)]
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_convergence_batch(None, C.byref(pp) if p else None, ptr(traces, dummy), ld, f.ctypes.data, B, ptr(ref_ts, dummy), ptr(ref_ls, dummy),
                                         *[ptr(on, c) for on, c in zip(curves, cur)], dummy.ctypes.data, dummy.ctypes.data, None)
    assert all((c == 99.0).all() for c in cur) and not dummy.any()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    assert hasattr(lib, "tspws_hip_convergence_batch") and hasattr(lib, "tspws_hip_convergence_batch_stats")
    assert "tspws_hip_convergence_batch" in tspws.SYMBOLS and "tspws_hip_convergence_batch_stats" in tspws.SYMBOLS
    for name in ("convergence", "convergence_batch", "convergence_batch_stats"):
        assert hasattr(tspws.Plan, name), name
    stats = (C.c_uint * 6)()
    assert lib.tspws_hip_convergence_batch_stats(None, C.byref(stats)) == -1


def test_header_declares_them():
    with open(os.path.join(abi.ROOT, "include", "tspws_hip.h")) as fh:
        text = fh.read()
    assert "tspws_hip_convergence_batch(" in text and "tspws_hip_convergence_batch_stats(" in text and "tspws_hip_conv_batch_stats;" in text


def test_null_arguments(lib):
    one = lambda i: tuple(j != i for j in range(4))  # noqa: E731
    cases = [dict(p=False), dict(traces=False), dict(ref_ts=False), dict(ref_ls=False)] + [dict(curves=one(i)) for i in range(4)] + [dict()]  # (the last: NULL plan)
    for kw in cases:
        rc, err = call(lib, **kw)
        assert rc == -1 and err.startswith(b"convergence_batch: NULL"), (kw, err)
    p = abi.default_params(Kmax=10)
    rc = lib.tspws_hip_convergence_batch(None, C.byref(p), None, 256, None, 2, None, None, None, None, None, None, None, None, None)  # NULL offsets
    assert rc == -1 and lib.tspws_hip_last_error().startswith(b"convergence_batch: NULL")
    # B == 0 does nothing, but a NULL plan is still an error
    f = np.array([0, 12, 24], dtype=np.uint64)
    assert lib.tspws_hip_convergence_batch(None, C.byref(p), None, 256, f.ctypes.data, 0, None, None, None, None, None, None, None, None, None) == -1


def test_decreasing_offsets(lib):
    rc, err = call(lib, first=(0, 16, 12))
    assert rc == -1 and err.startswith(b"convergence_batch: decreasing"), err
    # an empty ensemble is no decreasing offset: the NULL plan is what refuses
    rc, err = call(lib, first=(0, 24, 24))
    assert rc == -1 and err.startswith(b"convergence_batch: NULL"), err
