"""The checker of the real-weighted stacks (tspws_hip_weighted_stack_batch, Plan.weighted_stack_batch): the expected rows of a weight matrix,
the definition of include/tspws_hip.h applied literally in numpy FP64 on the repository's own oracle frame.  Per ensemble, with Y_i =
OracleFrame.forward of trace i and w_i the row's weights on its traces:
  a trace with w_i == 0 is skipped altogether; n+ = the traces with w_i > 0; W = sum w_i, Q = sum w_i^2 added one by one in trace order,
  Keff = W W / Q;
  ST += w_i Y_i and PS += w_i u_i in trace order (product, then sum: two roundings), u_i = (Re Y_i / r, Im Y_i / r) with r = hypot(Re, Im),
  a coefficient whose u_i is not a unit phasor (Y_i == 0: NaN) adding nothing to PS;
  OUT by the weight rule of the mode with (W, Keff): unbiased ST (Keff c^2 - 1) / (Keff - 1) / W with c = |PS| / W (n+ == 1 or Keff == 1: the
  biased wu == 2 rule), biased wu == 2 ST |PS|^2 / (W W W), wu == 1 ST |PS| / (W W), else ST (|PS| / W)^wu / W -- the expressions in the order of
  operations of the oracle's weight with (K, M) = (W, W), so that a 0/1 row has the bits of tests/boot_batch_ref.py;
  ts = (float32) OracleFrame.inverse(OUT); ls = a float32 accumulator, acc = (float32)((double)acc + w_i (double)x_i) over the participating
  traces in trace order, times (float32)(1 / W).
n+ == 0: zero rows, count 0, Keff 0.  (The library fuses product and sum of ST / PS into one rounding; both forms agree far inside the
parity tolerance and exactly for weights 0 and 1.)

The stacks of a row do not depend on the weight mode, and a row does not depend on the other rows: Stacks keeps the transforms of an
ensemble's traces and the (ST, PS, float accumulator, n+, W, Keff) of every distinct weight row, so that the tests share them."""
import math

import numpy as np

import abi


def row_sums(w):
    """(n+, W, Q, Keff) of one weight row: FP64 sums in trace order."""
    W = Q = 0.0
    for v in np.asarray(w, dtype=np.float64):
        v = float(v)
        W += v
        Q += v * v
    npos = int((np.asarray(w) > 0).sum())
    return npos, W, Q, (W * W / Q if npos else 0.0)


def cplx(re, im):
    """re + i im without an operation."""
    z = np.empty(len(re), np.complex128)
    z.real, z.imag = re, im
    return z


def weight(ST, PS, npos, W, Keff, wu, unbiased):
    """The weighted coefficients of one row (every product of a complex and a real number by components)."""
    re, im = PS.real, PS.imag
    if wu == 2 and unbiased and npos != 1 and Keff != 1:
        iK, iK1, iM = 1.0 / W, 1.0 / (Keff - 1), 1.0 / W
        pr, pi = re * iK, im * iK
        a = pr * pr + pi * pi
        a = (Keff * a - 1) * iK1
        return cplx(ST.real * a * iM, ST.imag * a * iM)
    if wu == 2:
        a = (re * re + im * im) * (1.0 / (W * W * W))
        return cplx(a * ST.real, a * ST.imag)
    if wu == 1:
        r, g = np.hypot(re, im), 1.0 / (W * W)
        return cplx(ST.real * r * g, ST.imag * r * g)
    a = np.hypot(re, im) / W
    a = np.array([math.pow(v, wu) for v in a])  # (libm's pow, element by element: what the oracle calls)
    return cplx(ST.real * a / W, ST.imag * a / W)


class Stacks:
    """The linear / phase stacks and float accumulators of weight rows over ONE ensemble (float32 [m][N]) in the frame of resolved params p."""

    def __init__(self, p, seg):
        self.seg = np.ascontiguousarray(seg, dtype=np.float32)
        self.N = self.seg.shape[1]
        self.frame = abi.OracleFrame.from_params(p, self.N)
        self.Y = [np.ascontiguousarray(self.frame.forward(x.astype(np.float64))) for x in self.seg]
        self.U = []
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for Y in self.Y:
                r = np.hypot(Y.real, Y.imag)
                ur, ui = Y.real / r, Y.imag / r
                ok = ur * ur + ui * ui <= 1.001  # (NaN fails)
                self.U.append((np.where(ok, ur, 0.0), np.where(ok, ui, 0.0)))
        self.rows = {}

    def row(self, w):
        """(ST, PS, acc, n+, W, Keff) of one weight row; cached by the row's bytes."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (len(self.seg),)
        key = w.tobytes()
        if key not in self.rows:
            nc = self.frame.ncoef
            sr, si, pr, pi = (np.zeros(nc) for _ in range(4))
            acc = np.zeros(self.N, np.float32)
            for i, wi in enumerate(w):
                if wi == 0:
                    continue
                sr, si = sr + wi * self.Y[i].real, si + wi * self.Y[i].imag
                pr, pi = pr + wi * self.U[i][0], pi + wi * self.U[i][1]
                acc = (acc.astype(np.float64) + wi * self.seg[i].astype(np.float64)).astype(np.float32)
            npos, W, _, Keff = row_sums(w)
            self.rows[key] = (cplx(sr, si), cplx(pr, pi), acc, npos, W, Keff)
        return self.rows[key]

    def replica(self, w, wu, unbiased):
        """(ls, ts, n+, Keff) of one weight row: float32 [N] each."""
        ST, PS, acc, npos, W, Keff = self.row(w)
        if not npos:
            return np.zeros(self.N, np.float32), np.zeros(self.N, np.float32), 0, 0.0
        OUT = weight(ST, PS, npos, W, Keff, float(wu), int(unbiased))
        ts = self.frame.inverse(OUT).astype(np.float32)
        ls = acc * np.float32(1.0 / W)
        return ls, ts, npos, Keff


def expected(p, X, first, w, stacks=None):
    """Expected ls[B][M][N], ts[B][M][N] (float32), n+[B][M] (uint32) and Keff[B][M] (float64) of the batch: ensemble b = rows [first[b],
    first[b+1]) of X, w [M][T] with column i - first[0] for trace i.  `stacks`: a dict that keeps the Stacks of every ensemble between calls
    (same X, first and frame)."""
    first = np.asarray(first, dtype=np.int64)
    B, M, N, f0 = len(first) - 1, w.shape[0], X.shape[1], int(first[0])
    ls, ts = np.zeros((B, M, N), np.float32), np.zeros((B, M, N), np.float32)
    K, keff = np.zeros((B, M), np.uint32), np.zeros((B, M), np.float64)
    stacks = {} if stacks is None else stacks
    for b in range(B):
        a, e = int(first[b]), int(first[b + 1])
        if e == a:
            continue
        if b not in stacks:
            stacks[b] = Stacks(p, X[a:e])
        for m in range(M):
            ls[b, m], ts[b, m], K[b, m], keff[b, m] = stacks[b].replica(w[m, a - f0:e - f0], p.wu, p.unbiased)
    return ls, ts, K, keff
