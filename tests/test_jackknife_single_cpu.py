"""Single-stage jackknife, host side (no GPU): the selection classes of tspws_selection_classes against np.unique, the Python helpers,
and a self-check of the trace-order restatement the GPU tests compare against."""
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


def classes_c(lib, sel):
    sel = np.ascontiguousarray(sel, np.int8)
    Cn, mtr = sel.shape
    cls = np.zeros(mtr, np.uint32)
    kept = np.full(Cn * max(mtr, 1), 7, np.int8)
    n = C.c_uint(12345)
    assert lib.tspws_selection_classes(sel.ctypes.data, Cn, mtr, cls.ctypes.data, kept.ctypes.data, C.byref(n)) == 0
    return cls, kept[:Cn * n.value].reshape(Cn, n.value)


def check_classes(lib, sel):
    cls, kept = classes_c(lib, sel)
    want_cls, want_kept = ref.classes_numpy(sel)
    np.testing.assert_array_equal(cls, want_cls)
    np.testing.assert_array_equal(kept, want_kept)
    return kept.shape[1]


@pytest.mark.parametrize("n,d,mtr", [(4, 1, 60), (5, 2, 200), (6, 5, 37), (12, 3, 499), (16, 3, 150)])
def test_classes_of_jackknife_plans(lib, n, d, mtr):
    times = ref.leap_times(mtr, seed=n * 10 + d)
    sel = ref.selection(times, n, d)
    ncls = check_classes(lib, sel)
    bins = np.floor(np.array([(np.datetime64(int(t), "s").astype("datetime64[D]") - np.datetime64(int(t), "s").astype("datetime64[Y]")).astype(int)
                              for t in times]) * n / 365.0).astype(int)
    assert ncls == len(np.unique(bins)) and ncls <= n + 1
    assert bins.max() == n  # the leap day's bin is there ...
    last = np.flatnonzero(bins == n)
    assert (sel[:, last] == 1).all()  # ... and never deleted


def test_classes_of_arbitrary_selections(lib):
    rng = np.random.default_rng(5)
    for Cn, mtr in ((1, 1), (3, 10), (8, 300), (40, 97), (130, 64)):
        check_classes(lib, (rng.random((Cn, mtr)) < 0.6).astype(np.int8))
    # all ones: one class kept by every replica
    cls, kept = classes_c(lib, np.ones((5, 33), np.int8))
    assert not cls.any() and kept.shape == (5, 1) and kept.all()
    # a class absent from some replica (and a replica with no trace at all)
    sel = np.ones((4, 20), np.int8)
    sel[1, 5:9] = 0
    sel[2, :] = 0
    assert check_classes(lib, sel) == 2  # traces 5..8 and the rest
    # bytes other than 1 count as "not kept" (the engine's rule: sel[i] == 1)
    sel2 = sel.copy()
    sel2[0, 0] = 2
    cls2, kept2 = classes_c(lib, sel2)
    want_cls, want_kept = ref.classes_numpy(sel2)
    np.testing.assert_array_equal(cls2, want_cls)
    np.testing.assert_array_equal(kept2, want_kept)
    # no traces: no classes; NULL arguments are refused
    cls, kept = classes_c(lib, np.zeros((3, 0), np.int8))
    assert kept.shape == (3, 0)
    assert lib.tspws_selection_classes(None, 1, 1, None, None, None) == -1


def test_python_helpers(lib):
    times = ref.leap_times(80, seed=1)
    sel = tspws.jackknife_selection(times, 5, 2)
    np.testing.assert_array_equal(sel, ref.selection(times, 5, 2))
    cls, kept = tspws.selection_classes(sel)
    want_cls, want_kept = ref.classes_numpy(sel)
    np.testing.assert_array_equal(cls, want_cls)
    np.testing.assert_array_equal(kept, want_kept)
    with pytest.raises(tspws.TspwsError):
        tspws.jackknife_selection(np.zeros(10, np.int64), 4, 1)  # no start times
    with pytest.raises(tspws.TspwsError):
        tspws.jackknife_selection(times, 4, 4)
    for name in ("tspws_selection_classes", "tspws_hip_jackknife_single"):
        assert name in tspws.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("kw,mtr,N", [(dict(), 12, 2048), (dict(type=-3, unbiased=1), 9, 1501), (dict(wu=1.3, lrm=1), 7, 3000)])
def test_restatement_all_ones_is_the_single_stage_stack(kw, mtr, N):
    X = abi.synth_traces(mtr, N, seed=4)
    p, Xp, r = ref.prologue(abi.default_params(**kw), X)
    ls, ts, K = ref.Restatement(p, Xp).replica(np.ones(mtr, np.int8))
    assert K == mtr
    assert abi.relerr(ts, r["tsPWS"]) < 1e-7
    # (the main stack's ls is the reconstruction of ST, :233-241; a replica's is the time-domain mean, :799-811)
    np.testing.assert_array_equal(ls, (Xp.astype(np.float64).sum(axis=0) * (1.0 / mtr)).astype(np.float32))
