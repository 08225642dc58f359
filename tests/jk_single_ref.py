"""Trace-order restatement of the single-stage jackknife (shared by tests/test_jackknife_single_*.py).

Replica c of a selection sel[C][mtr] is the single-stage resampling body (ts_pws1f_lib.c:501-610) on mask row c with K = M = K_c, built
here from the oracle's primitives: orc_forward of every trace, orc_accumulate over the selected traces in trace order, orc_weight(K_c,
K_c), orc_inverse; the linear stack is the FP64 sum of the selected traces times 1 / K_c.  A replica without traces gives zero rows.
"""
import ctypes as C
import datetime as dt

import numpy as np

import abi


def leap_times(mtr, seed=0):
    """Start times over two years (1 Jan 2015 .. 31 Dec 2016), sorted, with the last trace on 31 December 2016 (tm_yday 365 of a leap
    year: bin n, never deleted) and one more on 31 December at the middle of the ensemble."""
    rng = np.random.default_rng(seed)
    t0 = int(dt.datetime(2015, 1, 1, tzinfo=dt.timezone.utc).timestamp())
    leap = int(dt.datetime(2016, 12, 31, 6, tzinfo=dt.timezone.utc).timestamp())
    t = np.sort(t0 + rng.integers(0, 730 * 86400, mtr)).astype(np.int64)
    t[-1] = leap
    t[mtr // 2] = leap - 366 * 86400  # 31 Dec 2015 (tm_yday 364)
    return np.sort(t)


def selection(times, n, d):
    """Jackknife selection [C][mtr] from the oracle's JackknifePlans restatement."""
    Cn = abi.binomial(n, d)
    times = np.ascontiguousarray(times, np.int64)
    sel = np.zeros((Cn, times.size), np.int8)
    assert abi.oracle().orc_jackknife_plan(sel.ctypes.data, times.ctypes.data, times.size, d, n, Cn) == 0
    return sel


def classes_numpy(sel):
    """(class_of_trace, kept[C][ncls]) from np.unique over the selection columns, classes in order of first appearance."""
    cols = (np.asarray(sel) == 1).T.astype(np.int8)
    if not cols.shape[0]:
        return np.zeros(0, np.uint32), np.zeros((sel.shape[0], 0), np.int8)
    _, first, inv = np.unique(cols, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    cls = rank[np.asarray(inv).reshape(-1)].astype(np.uint32)
    kept = cols[first[order]].T.astype(np.int8)
    return cls, kept


def prologue(params, X, beg=0.0):
    """(resolved params, traces used) of a tspws_main call: the oracle's own prologue (fold, mean removal, Nmax)."""
    r = abi.run_main(abi.oracle().orc_tspws_main, params, X, beg=beg)
    assert r["rc"] == 0
    p = r["params"]
    mtr = p.Nmax if p.Nmax and p.Nmax < X.shape[0] else X.shape[0]
    return p, r["sigall"][:mtr], r


class Restatement:
    """Transforms every trace once (orc_forward); replicas on demand."""

    def __init__(self, p, X):
        self.p = p
        self.X = np.ascontiguousarray(X, np.float32)
        mtr, N = self.X.shape
        self.f = abi.OracleFrame.from_params(p, N)
        self.Y = np.stack([self.f.forward(self.X[i].astype(np.float64)) for i in range(mtr)]) if mtr else np.zeros((0, self.f.ncoef), np.complex128)

    def replica(self, mask):
        lib, nc, N = self.f.lib, self.f.ncoef, self.X.shape[1]
        idx = np.flatnonzero(np.asarray(mask) == 1)
        K = idx.size
        if not K:
            return np.zeros(N, np.float32), np.zeros(N, np.float32), 0
        ST = np.zeros(2 * nc)
        PS = np.zeros(2 * nc)
        for i in idx:  # trace order
            lib.orc_accumulate(ST.ctypes.data, PS.ctypes.data, self.Y[i].ctypes.data, nc)
        OUT = np.zeros(2 * nc)
        lib.orc_weight(OUT.ctypes.data, ST.ctypes.data, PS.ctypes.data, nc, K, K, C.c_double(self.p.wu), int(self.p.unbiased))
        ts = self.f.inverse(OUT.view(np.complex128)).astype(np.float32)
        ls = (self.X[idx].astype(np.float64).sum(axis=0) * (1.0 / K)).astype(np.float32)
        return ls, ts, K

    def replicas(self, sel):
        out = [self.replica(row) for row in sel]
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.uint32))
