"""CPU-side checks of the batched stack entry point (tspws_hip_stack_batch): the library refuses bad arguments before any device work,
so these run on a host without a GPU."""
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


def test_null_plan_and_params(lib):
    first = np.array([0, 4, 8], dtype=np.uint64)
    p = abi.default_params()
    assert lib.tspws_hip_stack_batch(None, C.byref(p), None, 256, first.ctypes.data, 2, None, None, None) == -1
    assert b"NULL" in lib.tspws_hip_last_error()
    assert lib.tspws_hip_stack_batch(None, None, None, 256, first.ctypes.data, 0, None, None, None) == -1
    stats = (C.c_uint * 6)()
    assert lib.tspws_hip_stack_batch_stats(None, C.byref(stats)) == -1


def test_binding_declares_the_entry_point(lib):
    assert "tspws_hip_stack_batch" in tspws.SYMBOLS and "tspws_hip_stack_batch_stats" in tspws.SYMBOLS
    assert hasattr(tspws.Plan, "stack_batch")
