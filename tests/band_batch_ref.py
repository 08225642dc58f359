"""The checker of the band-limited batched stack (tspws_hip_stack_batch_bands, Plan.stack_batch_bands): the expected rows, the definition of
include/tspws_hip.h applied literally in numpy FP64 on the repository's own oracle frame (it follows tests/weighted_batch_ref.py).  Per
ensemble of m traces, with the resolved parameters p:
  single-stage (Kmax == 0 or Kmax > m): Y_i = OracleFrame.forward of trace i; ST = sum Y_i and PS = sum u_i in trace order, u_i = (Re Y_i / r,
  Im Y_i / r) with r = hypot(Re, Im), a coefficient whose u_i is not a unit phasor (Y_i == 0: NaN) adding nothing; (K, M) = (m, m);
  two-stage (0 < Kmax <= m): the partial stacks P_g = FP64 sum, in trace order, of the traces i with floor(i Kmax / m) == g; ST / PS as above
  over Y_g = forward(P_g), g = 0 .. Kmax - 1; (K, M) = (Kmax, m);
  OUT by the weight rule of the mode, in the oracle's order of operations: unbiased (wu == 2, K != 1) ST (K c^2 - 1) / (K - 1) / M with
  c = |PS| / K; biased wu == 2 ST |PS|^2 / (K K M); wu == 1 ST |PS| / (K M); else ST (|PS| / K)^wu / M;
  for a band [a, e): the sets OUT and ST with every coefficient outside the scales a <= s < e set to zero, x = OracleFrame.inverse of the masked
  set and q = OracleFrame.inverse of -i times it;
  ts = (float32) x(OUT), ts_env = (float32) hypot(x, q); ls = (float32) x(ST) / (float32) m, ls_env = (float32) hypot(x, q)(ST) / (float32) m.
An empty ensemble and an empty band give zero rows.

The stacks of an ensemble do not depend on the bands: Ensemble keeps them, and expected() keeps the Ensembles in the dict it is given."""
import math

import numpy as np

import abi
from band_rows_ref import rotate
from weighted_batch_ref import cplx


def weight(ST, PS, K, M, wu, unbiased):
    """The weighted coefficients (every product of a complex and a real number by components)."""
    K, M = float(K), float(M)
    re, im = PS.real, PS.imag
    if wu == 2 and unbiased and K != 1:
        iK, iK1, iM = 1.0 / K, 1.0 / (K - 1), 1.0 / M
        pr, pi = re * iK, im * iK
        a = pr * pr + pi * pi
        a = (K * a - 1) * iK1
        return cplx(ST.real * a * iM, ST.imag * a * iM)
    if wu == 2:
        a = (re * re + im * im) * (1.0 / (K * K * M))
        return cplx(a * ST.real, a * ST.imag)
    if wu == 1:
        r, g = np.hypot(re, im), 1.0 / (K * M)
        return cplx(ST.real * r * g, ST.imag * r * g)
    a = np.hypot(re, im) / K
    a = np.array([math.pow(v, wu) for v in a])
    return cplx(ST.real * a / M, ST.imag * a / M)


class Ensemble:
    """(OUT, ST, m) of one ensemble (float32 [m][N]) in the frame of the resolved parameters p, and its band rows."""

    def __init__(self, p, seg, frame=None):
        seg = np.ascontiguousarray(seg, dtype=np.float32)
        self.m, self.N = seg.shape
        self.frame = frame or abi.OracleFrame.from_params(p, self.N)
        m, K = self.m, int(p.Kmax)
        if 0 < K <= m:
            rows = np.zeros((K, self.N))
            for i in range(m):
                rows[int(math.floor(float(i * K) / float(m)))] += seg[i].astype(np.float64)
        else:
            rows, K = seg.astype(np.float64), m
        nc = self.frame.ncoef
        sr, si, pr, pi = (np.zeros(nc) for _ in range(4))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for x in rows:
                Y = self.frame.forward(x)
                r = np.hypot(Y.real, Y.imag)
                ur, ui = Y.real / r, Y.imag / r
                ok = ur * ur + ui * ui <= 1.001  # (NaN fails)
                sr, si = sr + Y.real, si + Y.imag
                pr, pi = pr + np.where(ok, ur, 0.0), pi + np.where(ok, ui, 0.0)
        self.ST = cplx(sr, si)
        self.OUT = weight(self.ST, cplx(pr, pi), K, m, float(p.wu), int(p.unbiased))
        self.off = np.concatenate([[0], np.cumsum(self.frame.Ns.astype(np.int64))])

    def band(self, a, e):
        """(ls, ts, ls_env, ts_env) float32 [N] of the band [a, e)."""
        out = []
        for Yset, div in ((self.ST, True), (self.OUT, False)):
            Z = np.zeros_like(Yset)
            Z[self.off[a]: self.off[e]] = Yset[self.off[a]: self.off[e]]
            x, q = self.frame.inverse(Z), self.frame.inverse(rotate(Z))
            row, env = x.astype(np.float32), np.hypot(x, q).astype(np.float32)
            if div:
                row, env = row / np.float32(self.m), env / np.float32(self.m)
            out.append((row, env))
        return out[0][0], out[1][0], out[0][1], out[1][1]


def expected(p, X, first, bands, ensembles=None):
    """Expected ls, ts, ls_env, ts_env [B][R][N] (float32): ensemble b = rows [first[b], first[b+1]) of X.  `ensembles`: a dict that keeps the
    Ensemble of every b between calls (same X, first and parameters)."""
    first = np.asarray(first, dtype=np.int64)
    B, R, N = len(first) - 1, len(bands), X.shape[1]
    out = [np.zeros((B, R, N), np.float32) for _ in range(4)]
    ensembles = {} if ensembles is None else ensembles
    frame = None
    for b in range(B):
        a, e = int(first[b]), int(first[b + 1])
        if e == a:
            continue
        if b not in ensembles:
            ensembles[b] = Ensemble(p, X[a:e], frame)
        frame = ensembles[b].frame
        for r, (s0, s1) in enumerate(bands):
            if s1 > s0:
                for o, row in zip(out, ensembles[b].band(int(s0), int(s1))):
                    o[b, r] = row
    return out
