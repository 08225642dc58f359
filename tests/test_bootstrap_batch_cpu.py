"""CPU-side checks of the batched bootstrap (tspws_hip_bootstrap_batch / _cnt, tspws_bootstrap_plan / _batch): the library exports the entry
points and the binding declares them; the host draws, in a fresh process per seed (tests/fresh_bootstrap.py); every refusal that needs no
device, with sentinel-filled outputs unchanged and nothing drawn; and the checker's own test -- tests/boot_batch_ref.py against the oracle's
single-stage random subsampling on the same mask (a 0/1 count row) and on the gathered expanded ensemble (counts above 1)."""
import ctypes as C
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import boot_batch_ref as bbr

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))

NAMES = ("tspws_bootstrap_plan", "tspws_bootstrap_plan_batch", "tspws_hip_bootstrap_batch_cnt", "tspws_hip_bootstrap_batch",
         "tspws_hip_bootstrap_batch_stats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def call(lib, drawing=False, p=True, first=(0, 6, 9), cnt=True, Mn=3, ls_out=True, ts_out=True, mtr_out=True, ld=256, x=True, B=None, Kmax=10, stats=False):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    f = np.array(first, dtype=np.uint64) if first is not None else None
    B = (f.size - 1 if f is not None else 2) if B is None else B
    c = np.ones((Mn, 9), np.uint8)
    pp = abi.default_params(Kmax=Kmax)
    dummy = np.full(16, 7.0, np.float32)
    m = np.full(max(1, B * Mn), 99, np.uint32)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    head = (None, C.byref(pp) if p else None, ptr(x, dummy), ld, ptr(f is not None, f) if f is not None else None, B, Mn)
    tail = (ptr(ls_out, dummy), ptr(ts_out, dummy), ptr(mtr_out, m), ptr(stats, dummy), None)
    abi.srand(11)
    r0 = C.CDLL(None).rand()
    abi.srand(11)
    if drawing:
        rc = lib.tspws_hip_bootstrap_batch(*head, *tail)
    else:
        rc = lib.tspws_hip_bootstrap_batch_cnt(*head, ptr(cnt, c), *tail)
    assert (m == 99).all() and (dummy == 7.0).all()  # outputs untouched
    assert C.CDLL(None).rand() == r0                 # ... and a refused call draws nothing
    return rc, lib.tspws_hip_last_error()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("bootstrap_batch", "bootstrap_batch_stats"):
        assert hasattr(tspws.Plan, n), n
    assert hasattr(tspws, "bootstrap_counts_batch")
    stats = (C.c_uint * 5)()
    assert lib.tspws_hip_bootstrap_batch_stats(None, C.byref(stats)) == -1
    assert b"bootstrap_batch_stats: NULL" in lib.tspws_hip_last_error()


@pytest.mark.parametrize("seed", [1, 77])
def test_host_draws_in_a_fresh_process(lib, seed):
    out = subprocess.run([sys.executable, os.path.join(HERE, "fresh_bootstrap.py"), str(seed)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"FRESH_BOOTSTRAP OK {seed}" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize("drawing", [False, True])
def test_null_arguments(lib, drawing):
    cases = [dict(p=False), dict(first=None), dict(ls_out=False), dict(ts_out=False), dict(mtr_out=False), dict(), dict(stats=True)]  # (the last two: NULL plan)
    if not drawing:
        cases.append(dict(cnt=False))
    for kw in cases:
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"bootstrap_batch: NULL" in err, (kw, err)
    # B == 0 / M == 0 do nothing, but a NULL plan is still an error (as in the other batch calls; tests/test_bootstrap_batch_gpu.py has them with
    # a plan: they return 0)
    for kw in (dict(B=0), dict(Mn=0)):
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"bootstrap_batch: NULL" in err, (kw, err)
    # ... and NULL p / h_first are refused even then
    for kw in (dict(B=0, p=False), dict(Mn=0, p=False)):
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"bootstrap_batch: NULL" in err, (kw, err)


@pytest.mark.parametrize("drawing", [False, True])
def test_inconsistent_arguments(lib, drawing):
    rc, err = call(lib, drawing=drawing, first=(0, 8, 6))
    assert rc == -1 and b"bootstrap_batch: decreasing" in err, err
    # a two-stage ensemble needs no plan to be seen: Kmax = 2 <= 5 traces; so does one beside an empty and a single-stage ensemble
    for first in ((0, 5), (0, 0, 1, 9)):
        rc, err = call(lib, drawing=drawing, first=first, Kmax=2)
        assert rc == -1 and b"bootstrap_batch: " in err and b"two-stage" in err, err
    # ... while Kmax above every ensemble (or 0) is single-stage: only the NULL plan refuses
    for kmax in (0, 7):
        rc, err = call(lib, drawing=drawing, Kmax=kmax)
        assert rc == -1 and b"bootstrap_batch: NULL" in err, err
    # NULL traces and a short row stride need the plan's trace length, so that the NULL plan is what refuses them here
    # (tests/test_bootstrap_batch_gpu.py has them with a plan)
    for kw in (dict(x=False), dict(ld=3)):
        rc, err = call(lib, drawing=drawing, **kw)
        assert rc == -1 and b"bootstrap_batch: NULL" in err, (kw, err)


def test_binding_refuses_bad_counts():
    with pytest.raises(tspws.TspwsError):
        tspws.bootstrap_counts_batch([0, 5, 4], 2)
    with pytest.raises(tspws.TspwsError):
        tspws.bootstrap_counts_batch([[0, 5]], 2)
    assert tspws.bootstrap_counts_batch([2, 7], 3).shape == (3, 5)


# ---- the checker's own test ------------------------------------------------------------------------------------------------------------------
N, MTR = 256, 7
KW = [dict(), dict(unbiased=1), dict(wu=1.5, type=-3)]


def oracle_subsamples(kw, X, M, prob, seed):
    """(sub_ls, sub_ts, masks) of the oracle's single-stage random subsampling of X: tspws_main after srand(seed), and the masks it drew."""
    abi.srand(seed)
    w = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(subsmpl_N=M, subsmpl_p=prob, **kw), X)
    assert w["rc"] == 0
    K = math.ceil(len(X) * prob)
    sel = np.zeros((M, len(X)), np.int8)
    abi.srand(seed)
    for m in range(M):
        assert abi.oracle().orc_subsampling_plan(sel[m].ctypes.data, len(X), K) == 0
    return w["sub_ls"], w["sub_ts"], sel


@pytest.mark.parametrize("kw", KW, ids=["biased", "unbiased", "wu1.5-mexhat"])
def test_checker_on_masks_is_the_subsample_reference(kw):
    """A 0/1 count row: the checker's rows are the oracle's subsamples on the same masks (the reference of tests/sub_batch_engine.py), bit for
    bit -- the same pieces in the same order."""
    X = abi.synth_traces(MTR, N, seed=4)
    M, prob = 3, 0.5
    wl, wt, sel = oracle_subsamples(kw, X, M, prob, seed=21)
    assert ((sel == 1).sum(axis=1) == math.ceil(MTR * prob)).all() and len({r.tobytes() for r in sel}) > 1
    p = abi.resolve(abi.default_params(**kw), N)
    ls, ts, K = bbr.expected(p, X, [0, MTR], sel.astype(np.uint8))
    assert (K == math.ceil(MTR * prob)).all()
    assert (np.abs(wl).max(axis=1) > 0).all() and (np.abs(wt).max(axis=1) > 0).all()
    np.testing.assert_array_equal(ls[0], wl)
    np.testing.assert_array_equal(ts[0], wt)


@pytest.mark.parametrize("kw", KW, ids=["biased", "unbiased", "wu1.5-mexhat"])
def test_checker_on_counts_is_the_subsample_of_the_expanded_ensemble(kw):
    """Counts above 1: the checker's row is the oracle's subsample, with every trace kept (prob 1), of the gathered expanded array; among the
    rows a single copy (the K = 1 rule) and an empty row."""
    X = abi.synth_traces(MTR + 2, N, seed=9)
    first = [2, 2 + MTR]
    cnt = np.array([[0, 3, 1, 0, 2, 1, 0], [5, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 255]], np.uint8)
    p = abi.resolve(abi.default_params(**kw), N)
    ls, ts, K = bbr.expected(p, X, first, cnt)
    np.testing.assert_array_equal(K[0], cnt.astype(np.int64).sum(axis=1))
    for m in range(len(cnt)):
        if not K[0, m]:
            assert not ls[0, m].any() and not ts[0, m].any()
            continue
        Xe = bbr.expand(X[2:], cnt[m])
        assert len(Xe) == K[0, m]
        wl, wt, sel = oracle_subsamples(kw, Xe, 1, 1.0, seed=3)
        assert (sel == 1).all() and np.abs(wl[0]).max() > 0 and np.abs(wt[0]).max() > 0
        np.testing.assert_array_equal(ls[0, m], wl[0])
        np.testing.assert_array_equal(ts[0, m], wt[0])
