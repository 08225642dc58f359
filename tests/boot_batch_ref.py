"""The checker of the batched bootstrap (tspws_hip_bootstrap_batch_cnt, Plan.bootstrap_batch): the expected rows of a count matrix from the
EXPANDED ensemble -- the traces of an ensemble in trace order, trace i repeated cnt[m][i] times -- with the oracle's pieces: orc_forward per
trace (a copy's transform is its trace's), orc_accumulate once per copy in trace order, orc_weight(K, K, wu, unbiased), orc_inverse and a float
cast; the linear row is a float32 accumulator with the reference's double round trip, acc = (float)((double)acc + (double)x) once per copy,
times (float)(1. / K).  K = 0: zero rows.  Only the repository's own oracle is used.

The stacks of a row do not depend on the weight mode, and a row does not depend on the other rows: Stacks keeps the transforms of an
ensemble's traces and the (ST, PS, float accumulator) of every distinct count row, so that the tests share them."""
import numpy as np

import abi


class Stacks:
    """The linear / phase stacks and float accumulators of count rows over ONE ensemble (float32 [m][N]) in the frame of resolved params p."""

    def __init__(self, p, seg):
        self.seg = np.ascontiguousarray(seg, dtype=np.float32)
        self.N = self.seg.shape[1]
        self.frame = abi.OracleFrame.from_params(p, self.N)
        self.Y = [np.ascontiguousarray(self.frame.forward(x.astype(np.float64))) for x in self.seg]
        self.rows = {}

    def row(self, counts):
        """(ST, PS, acc, K) of one count row; cached by the row's bytes."""
        counts = np.asarray(counts, dtype=np.uint8)
        assert counts.shape == (len(self.seg),)
        key = counts.tobytes()
        if key not in self.rows:
            orc, nc = abi.oracle(), self.frame.ncoef
            ST, PS = np.zeros(nc, np.complex128), np.zeros(nc, np.complex128)
            acc = np.zeros(self.N, np.float32)
            for i, c in enumerate(counts):
                x64 = self.seg[i].astype(np.float64)
                for _ in range(int(c)):  # one addition per copy, in trace order
                    orc.orc_accumulate(ST.ctypes.data, PS.ctypes.data, self.Y[i].ctypes.data, nc)
                    acc = (acc.astype(np.float64) + x64).astype(np.float32)
            self.rows[key] = (ST, PS, acc, int(counts.astype(np.int64).sum()))
        return self.rows[key]

    def replica(self, counts, wu, unbiased):
        """(ls, ts, K) of one count row: float32 [N] each."""
        ST, PS, acc, K = self.row(counts)
        if not K:
            return np.zeros(self.N, np.float32), np.zeros(self.N, np.float32), 0
        OUT = np.zeros(self.frame.ncoef, np.complex128)
        abi.oracle().orc_weight(OUT.ctypes.data, ST.ctypes.data, PS.ctypes.data, self.frame.ncoef, K, K, float(wu), int(unbiased))
        ts = self.frame.inverse(OUT).astype(np.float32)
        ls = acc * np.float32(1.0 / K)
        return ls, ts, K


def expected(p, X, first, cnt, stacks=None):
    """Expected ls[B][M][N], ts[B][M][N] (float32) and K[B][M] (uint32) of the batch: ensemble b = rows [first[b], first[b+1]) of X, cnt [M][T]
    with column i - first[0] for trace i.  `stacks`: a dict that keeps the Stacks of every ensemble between calls (same X, first and frame)."""
    first = np.asarray(first, dtype=np.int64)
    B, M, N, f0 = len(first) - 1, cnt.shape[0], X.shape[1], int(first[0])
    ls, ts, K = np.zeros((B, M, N), np.float32), np.zeros((B, M, N), np.float32), np.zeros((B, M), np.uint32)
    stacks = {} if stacks is None else stacks
    for b in range(B):
        a, e = int(first[b]), int(first[b + 1])
        if e == a:
            continue
        if b not in stacks:
            stacks[b] = Stacks(p, X[a:e])
        for m in range(M):
            ls[b, m], ts[b, m], K[b, m] = stacks[b].replica(cnt[m, a - f0:e - f0], p.wu, p.unbiased)
    return ls, ts, K


def expand(seg, counts):
    """The expanded ensemble as an array: trace i of seg repeated counts[i] times, in trace order."""
    return np.ascontiguousarray(np.repeat(seg, np.asarray(counts, dtype=np.int64), axis=0))
