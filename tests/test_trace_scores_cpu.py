"""CPU-side checks of the trace scores and the selective stack (tspws_hip_trace_scores, tspws_selection_from_scores,
tspws_hip_selective_stack_batch): the library exports the entry points and the binding declares them; every refusal that needs no device,
with a NULL plan, host dummies and sentinel-filled outputs unchanged; the host rule against its numpy restatement
(tests/trace_scores_ref.py), bit for bit; and the checker's own test -- its longdouble sums against np.dot in FP64, inside its own bounds."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import abi
import trace_scores_ref as tsr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_trace_scores", "tspws_hip_trace_scores_stats", "tspws_selection_from_scores", "tspws_hip_selective_stack_batch")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("trace_scores", "trace_scores_stats", "selective_stack_batch"):
        assert hasattr(tspws.Plan, n), n
    assert callable(tspws.selection_from_scores)
    stats = (C.c_uint * 4)()
    assert lib.tspws_hip_trace_scores_stats(None, C.byref(stats)) == -1
    assert b"trace_scores_stats: NULL" in lib.tspws_hip_last_error()


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------
def scores_call(lib, traces=True, first=(2, 5, 5, 9), fptr=True, refs=True, scores=True, energy=True, ld=256, ldr=256, R=2, n0=0, n1=0, B=None):
    """One tspws_hip_trace_scores call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is
    refused before device work)."""
    dummy = np.full(16, 7.0, np.float32)
    ref = np.full(16, 5.0, np.float32)
    out = np.full(64, -3.0)
    en = np.full(16, -4.0)
    f = np.array(first, dtype=np.uint64)
    rc = lib.tspws_hip_trace_scores(None, dummy.ctypes.data if traces else None, ld, f.ctypes.data if fptr else None, f.size - 1 if B is None else B,
                                    ref.ctypes.data if refs else None, ldr, R, n0, n1, out.ctypes.data if scores else None,
                                    en.ctypes.data if energy else None, None)
    assert (out == -3.0).all() and (en == -4.0).all() and (dummy == 7.0).all() and (ref == 5.0).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_trace_scores_refusals(lib):
    # the NULL plan itself, with everything else in order (also without an energy output and with R = 1 .. 4)
    for kw in (dict(), dict(energy=False), dict(R=1), dict(R=3), dict(R=4), dict(n0=3, n1=9), dict(traces=False), dict(ld=3), dict(ldr=3), dict(n1=10 ** 9)):
        rc, err = scores_call(lib, **kw)  # (NULL traces, short strides and a window past max need the plan: the NULL plan is what refuses them here)
        assert rc == -1 and b"trace_scores: NULL" in err, (kw, err)
    for kw in (dict(fptr=False), dict(refs=False), dict(scores=False)):
        rc, err = scores_call(lib, **kw)
        assert rc == -1 and b"trace_scores: NULL" in err, (kw, err)
    # B == 0 does nothing, but a NULL plan is still an error (tests/test_trace_scores_gpu.py has it with a plan: 0)
    rc, err = scores_call(lib, B=0)
    assert rc == -1 and b"trace_scores: NULL" in err, err
    # what needs no plan comes first
    for R in (0, 5, 100):
        rc, err = scores_call(lib, R=R)
        assert rc == -1 and b"trace_scores: 1 to 4 reference rows" in err, (R, err)
    for n0, n1 in ((5, 5), (9, 3), (1, 1)):
        rc, err = scores_call(lib, n0=n0, n1=n1)
        assert rc == -1 and b"trace_scores: an empty lag window" in err, (n0, n1, err)
    rc, err = scores_call(lib, first=(2, 5, 4, 9))
    assert rc == -1 and b"trace_scores: decreasing ensemble offsets" in err, err


def selective_call(lib, params=True, traces=True, first=(2, 5, 5, 9), fptr=True, ls=True, ts=True, sel=True, kept=True, done=True, ld=256, against=1, rule=1,
                   a=3.0, iters=2, n0=0, n1=0, B=None):
    """One tspws_hip_selective_stack_batch call with a NULL plan and host dummies."""
    p = abi.default_params()
    dummy = np.full(16, 7.0, np.float32)
    o_ls, o_ts = np.full(16, -3.0, np.float32), np.full(16, -5.0, np.float32)
    h_sel = np.full(16, 9, np.int8)
    h_kept = np.full(4, 77, np.uint32)
    n_done = C.c_uint(1234)
    f = np.array(first, dtype=np.uint64)
    rc = lib.tspws_hip_selective_stack_batch(None, C.byref(p) if params else None, dummy.ctypes.data if traces else None, ld, f.ctypes.data if fptr else None,
                                             f.size - 1 if B is None else B, against, rule, a, iters, n0, n1, o_ls.ctypes.data if ls else None,
                                             o_ts.ctypes.data if ts else None, h_sel.ctypes.data if sel else None, h_kept.ctypes.data if kept else None,
                                             C.byref(n_done) if done else None, None)
    assert (o_ls == -3.0).all() and (o_ts == -5.0).all() and (h_sel == 9).all() and (h_kept == 77).all() and n_done.value == 1234 and (dummy == 7.0).all()
    return rc, lib.tspws_hip_last_error()


def test_selective_stack_refusals(lib):
    for kw in (dict(), dict(done=False), dict(against=0), dict(rule=0, a=-2.0), dict(iters=1), dict(traces=False), dict(ld=3), dict(n1=10 ** 9), dict(B=0)):
        rc, err = selective_call(lib, **kw)  # (the NULL plan)
        assert rc == -1 and b"selective_stack_batch: NULL" in err, (kw, err)
    for kw in (dict(params=False), dict(fptr=False), dict(ls=False), dict(ts=False), dict(sel=False), dict(kept=False)):
        rc, err = selective_call(lib, **kw)
        assert rc == -1 and b"selective_stack_batch: NULL" in err, (kw, err)
    for against in (-1, 2):
        rc, err = selective_call(lib, against=against)
        assert rc == -1 and b"selective_stack_batch: against" in err, (against, err)
    for kw in (dict(rule=2), dict(rule=-1), dict(a=float("nan")), dict(rule=0, a=float("nan"))):
        rc, err = selective_call(lib, **kw)
        assert rc == -1 and b"selective_stack_batch: an unknown rule or a NaN threshold" in err, (kw, err)
    rc, err = selective_call(lib, iters=0)
    assert rc == -1 and b"selective_stack_batch: iters == 0" in err, err
    rc, err = selective_call(lib, n0=7, n1=7)
    assert rc == -1 and b"selective_stack_batch: an empty lag window" in err, err
    rc, err = selective_call(lib, first=(2, 5, 4, 9))
    assert rc == -1 and b"selective_stack_batch: decreasing ensemble offsets" in err, err


# ---- the host rule ---------------------------------------------------------------------------------------------------------------------------
def rule_call(lib, score, first, rule, a, kept=True):
    f = np.array(first, dtype=np.uint64)
    T = int(f[-1] - f[0])
    sel = np.full(T + 2, 9, np.int8)  # a guard byte on either side
    k = np.full(f.size - 1 + 2, 77, np.uint32)
    sc = np.ascontiguousarray(score, dtype=np.float64)
    rc = lib.tspws_selection_from_scores(sel[1:].ctypes.data, k[1:].ctypes.data if kept else None, sc.ctypes.data, f.ctypes.data, f.size - 1, rule, a)
    assert sel[0] == 9 and sel[-1] == 9 and k[0] == 77 and k[-1] == 77
    return rc, sel[1:-1], k[1:-1]


def rule_scores(seed):
    """Scores of ensembles of 7 (odd), 8 (even), 0, 1, 2, 5 (all NaN) and 6 traces, first[0] = 3: similarities in [-1, 1], NaN among them,
    one +inf and one -inf (not finite: out of the median, still compared)."""
    rng = np.random.default_rng(seed)
    sizes = [7, 8, 0, 1, 2, 5, 6]
    first = 3 + np.concatenate([[0], np.cumsum(sizes)])
    s = rng.uniform(-1, 1, int(first[-1] - first[0]))
    s[[2, 9, 12]] = np.nan
    s[18:23] = np.nan  # the ensemble of 5
    s[24], s[26] = np.inf, -np.inf
    return s, first


def test_selection_rule_against_numpy(lib):
    for seed in range(4):
        s, first = rule_scores(seed)
        for rule, As in ((0, (-2.0, 0.0, 0.3, 2.0, float("inf"), -float("inf"))), (1, (0.0, 0.5, 1.0, 3.0, -1.0, float("inf")))):
            for a in As:
                rc, sel, kept = rule_call(lib, s, first, rule, a)
                want_sel, want_kept = tsr.select(s, first, rule, a)
                assert rc == 0 and np.array_equal(sel, want_sel) and np.array_equal(kept, want_kept), (seed, rule, a)
                assert not sel[np.isnan(s)].any()  # NaN is never kept
                assert kept[2] == 0 and kept[5] == 0  # the empty and the all-NaN ensemble
                rc, sel2, k2 = rule_call(lib, s, first, rule, a, kept=False)
                assert rc == 0 and np.array_equal(sel2, sel) and (k2 == 77).all()
    # the binding's wrapper
    s, first = rule_scores(9)
    sel, kept = tspws.selection_from_scores(s, first, "mad", 1.0)
    w_sel, w_kept = tsr.select(s, first, 1, 1.0)
    assert sel.dtype == np.int8 and kept.dtype == np.uint32 and np.array_equal(sel, w_sel) and np.array_equal(kept, w_kept)
    sel, kept = tspws.selection_from_scores(s, first, "threshold", 0.1)
    assert np.array_equal(sel, tsr.select(s, first, 0, 0.1)[0])


def test_selection_rule_ties_and_small_ensembles(lib):
    # ties at the threshold are kept (>=): rule 0 at a score itself; rule 1 with a = 0 keeps the median and what lies above it
    s = np.array([0.25, 0.5, 0.5, 0.75, 0.5])
    rc, sel, kept = rule_call(lib, s, [0, 5], 0, 0.5)
    assert rc == 0 and sel.tolist() == [0, 1, 1, 1, 1] and kept.tolist() == [4]
    rc, sel, kept = rule_call(lib, s, [0, 5], 1, 0.0)
    assert rc == 0 and sel.tolist() == [0, 1, 1, 1, 1]
    # (med = 0.5, mad = 0 there: every a gives the threshold 0.5); a = 1 with mad > 0 landing ON a score: sorted 1, 1.5174, 2, 3, 3, 4, 4.5 has
    # med 3, the deviations 0, 0, 1, 1, 1.4826, 1.5, 2 have mad 1, so the threshold is 3 - 1 * 1.4826 * 1, the second score itself
    t = np.array([3.0 - 1.0 * 1.4826 * 1.0, 1.0, 2.0, 3.0, 4.0, 4.5, 3.0])
    rc, sel, kept = rule_call(lib, t, [0, 7], 1, 1.0)
    w_sel, _ = tsr.select(t, [0, 7], 1, 1.0)
    assert rc == 0 and np.array_equal(sel, w_sel) and sel.tolist() == [1, 0, 1, 1, 1, 1, 1]
    # ensembles of 0, 1 and 2 traces, even median = 0.5 * (lo + hi)
    rc, sel, kept = rule_call(lib, [0.3, 0.1, 0.2], [4, 4, 5, 7], 1, 0.0)
    assert rc == 0 and sel.tolist() == [1, 0, 1] and kept.tolist() == [0, 1, 1]  # (0.1, 0.2): med 0.15, mad 0.05 (up to rounding), a = 0
    rc, sel, kept = rule_call(lib, [0.3, 0.1, 0.2], [4, 4, 5, 7], 1, 1.0)
    assert rc == 0 and sel.tolist() == [1, 1, 1] and kept.tolist() == [0, 1, 2]


def test_selection_rule_return_codes(lib):
    s = np.array([0.1, 0.2, 0.3])
    f = np.array([0, 3], np.uint64)
    sel = np.full(3, 9, np.int8)
    kept = np.full(1, 77, np.uint32)
    fn = lib.tspws_selection_from_scores
    assert fn(None, kept.ctypes.data, s.ctypes.data, f.ctypes.data, 1, 0, 0.0) == 1
    assert fn(sel.ctypes.data, kept.ctypes.data, None, f.ctypes.data, 1, 0, 0.0) == 1
    assert fn(sel.ctypes.data, kept.ctypes.data, s.ctypes.data, None, 1, 0, 0.0) == 1
    bad = np.array([0, 3, 2], np.uint64)
    assert fn(sel.ctypes.data, kept.ctypes.data, s.ctypes.data, bad.ctypes.data, 2, 0, 0.0) == 1
    for rule, a in ((2, 0.0), (-1, 0.0), (0, float("nan")), (1, float("nan"))):
        assert fn(sel.ctypes.data, kept.ctypes.data, s.ctypes.data, f.ctypes.data, 1, rule, a) == 2
    assert (sel == 9).all() and (kept == 77).all()  # nothing written
    assert fn(sel.ctypes.data, kept.ctypes.data, s.ctypes.data, f.ctypes.data, 1, 0, 0.15) == 0 and sel.tolist() == [0, 1, 1] and kept[0] == 2


# ---- the checker's own test ------------------------------------------------------------------------------------------------------------------
def test_checker_against_fp64_dot():
    """np.dot / np.sum in FP64 are FP64 summations in some order: they must lie inside the checker's bounds around its longdouble sums."""
    rng = np.random.default_rng(11)
    N, first = 1501, np.array([1, 6, 6, 9])
    x = (rng.standard_normal((10, N)) * 10.0 ** rng.uniform(-3, 3, (10, 1))).astype(np.float32)
    x[3] = 0  # a dead trace
    refs = rng.standard_normal((3, 2, N)).astype(np.float32)
    refs[2, 1] = 0  # a dead reference
    for win in (None, (3, 1499), (700, 701)):
        want = tsr.reference(x, first, refs, win)
        n0, n1 = tsr.window(N, win)
        T = 8
        scores = np.zeros((2, 3, T))
        energy = np.zeros(T)
        for b in range(3):
            for i in range(first[b], first[b + 1]):
                xd = x[i, n0:n1].astype(np.float64)
                energy[i - 1] = np.dot(xd, xd)
                for k in range(2):
                    rd = refs[b, k, n0:n1].astype(np.float64)
                    dot = np.dot(xd, rd)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        scores[k, 0, i - 1] = dot / np.sqrt(np.dot(xd, xd)) / np.sqrt(np.dot(rd, rd))
                    scores[k, 1, i - 1] = np.sum((xd - rd) ** 2)
                    scores[k, 2, i - 1] = dot
        tsr.check(scores, energy, want, f"fp64 numpy, window {win}")
        nan = np.isnan(scores[:, 0])
        assert nan[:, 2].all() and nan[1, 5:].all() and nan.sum() == 2 + 3 - 0  # trace 3 (column 2) for both references, ensemble 2 against its dead row
    # a wrong value is caught: one ulp-scale error times the window length is outside
    want = tsr.reference(x, first, refs, None)
    bad = np.stack([np.stack([want["sim"][k], want["misfit"][k], want["dot"][k]]) for k in range(2)]).astype(np.float64)
    bad[0, 1, 0] *= 1 + 4 * (N + 3) * tsr.U
    with pytest.raises(AssertionError):
        tsr.check(bad, None, want, "perturbed")
