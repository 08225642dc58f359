"""CPU reference for the stack's coherence filter per trace (tspws_hip_filter_coef, tspws_hip_filter_traces) with a bound at every
coefficient, and the checker that holds device sets to it (tests/test_filter_traces_gpu.py; the checker itself is tested in
tests/test_filter_traces_cpu.py).  No GPU import here.

From coefficient sets Y[M][ncoef] of one ensemble, in np.longdouble:

    PS   = sum_i u_i,  u_i = Y_i / |Y_i|, nothing where Y_i == 0 exactly (the reference's skip rule, ts_pws1f_lib.c:489-492)
    W    = the stack's weight without its ST and 1 / M factors, by the mode of (wu, unbiased, K) (ts_pws1f_lib.c:226-228, :972):
           0: |PS|^2 / K^2    1: |PS| / K    2: (|PS| / K)^wu    3: (K c - 1) / (K - 1), c = |PS / K|^2
    Y W  = the filtered set;   leave-one-out: W_i from PS - u_i and K - 1 (u_i subtracted only where the rule added it)

The bound per coefficient is an operation count times EPS = 2^-52 (inverse_rows_ref.EPS: twice the unit roundoff, which pays for the second
order) times the magnitudes of the terms; it uses no number of its own.  The device rounds every operation on its own, in the order that
include/tspws_hip.h states:

    mode 0   x x, y y, +, K K, 1 / (.), (.) g                        6 roundings of W,  |W| the magnitude
    mode 1   hypot (x x, y y, +, sqrt: 4), 1 / K, (.) g              6
    mode 3   1 / K, 1 / (K - 1), px, py (2 each: 5 per square), +, K c, - 1, (.) iK1:
             |dW| <= u (7 K c + 3 |K c - 1|) / (K - 1) <= 10 u (K c + 1) / (K - 1): 10 roundings on the ABSOLUTE term (K c + 1) / (K - 1)
    Y W      one more rounding per component

so |d(Y W)| <= (n + 1) EPS mag |Y| with n = 6, 6, 10.  Mode 2 goes through the device's pow, which has no stated bound here: it is held to
the project's parity tolerance (PARITY = 2e-6 of the largest |Y W| of the row) instead.  Under leave-one-out the phasor u_i that the device
recomputes carries the error term tests/stack_planes_ref.py allows per phasor of the phase stack (2^-50), and the subtraction one rounding
per component:  d|q| <= 2^-50 + EPS |q|, q = PS - u_i, which reaches W through dW / d|q| (2 |q| / K'^2, 1 / K', 2 |q| / (K' (K' - 1)))."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import inverse_rows_ref as irr

LD = np.longdouble
CLD = np.clongdouble
EPS = irr.EPS
PHASOR = LD(2.0 ** -50)       # stack_planes_ref's term per phasor of the phase stack
PARITY = 2e-6                 # the project's parity tolerance (relerr)
NOPS = {0: 6, 1: 6, 3: 10}


def weight_mode(wu, unbiased, K):
    """tspws_weight_mode (ts_pws1f_lib.c:226-228; K == 1 falls back to the biased weight, :972)."""
    if wu == 2 and unbiased and K != 1:
        return 3
    if wu == 2:
        return 0
    if wu == 1:
        return 1
    return 2


def phasors(Y):
    """u[M][ncoef] (clongdouble): Y / |Y|, 0 where Y == 0 exactly."""
    Yl = np.asarray(Y).astype(CLD)
    mag = np.abs(Yl)
    nz = np.asarray(Y) != 0
    return np.where(nz, Yl / np.where(nz, mag, LD(1)), 0)


def phase_stack(Y):
    """PS[ncoef] (clongdouble) of the sets Y[M][ncoef] by the skip rule, added trace by trace."""
    PS = np.zeros(np.asarray(Y).shape[1], CLD)
    for i in range(len(Y)):
        PS += phasors(Y[i:i + 1])[0]
    return PS


def weight(PS, K, mode, wu):
    """(W, mag) as longdouble arrays: the weight and the magnitude its rounding errors scale with."""
    PS = np.asarray(PS).astype(CLD)
    K = LD(K)
    r = np.abs(PS)
    if mode == 0:
        W = (r / K) ** 2
        return W, W
    if mode == 1:
        W = r / K
        return W, W
    if mode == 2:
        W = (r / K) ** LD(wu)
        return W, W
    c = (r / K) ** 2
    return (K * c - 1) / (K - 1), (K * c + 1) / (K - 1)


def _dW(r, K, mode, wu):
    """|dW / d|PS|| at |PS| = r."""
    K = LD(K)
    if mode == 0:
        return 2 * r / K ** 2
    if mode == 1:
        return np.full_like(r, 1 / K)
    if mode == 2:
        return LD(wu) * (r / K) ** (LD(wu) - 1) / K
    return 2 * r / (K * (K - 1))


class FilterRef:
    """want[M][ncoef] (clongdouble), bound[M][ncoef] (longdouble; None under mode 2), W ([ncoef], or [M][ncoef] under leave-one-out), the
    mode and the count in force."""

    def __init__(self, want, bound, W, mode, K):
        self.want, self.bound, self.W, self.mode, self.K = want, bound, W, mode, K


def reference(Y, PS, K, wu, unbiased, loo=False):
    """The filtered sets of the rows Y[M][ncoef] (complex128: the bits the device reads) of ONE ensemble with the phase stack PS[ncoef]
    (complex128: the bits the device reads) and the count K.  loo: row i with the weight of PS - u_i and K - 1."""
    Y = np.asarray(Y)
    assert Y.ndim == 2 and Y.dtype == np.complex128 and np.asarray(PS).dtype == np.complex128
    Yl = Y.astype(CLD)
    aY = np.abs(Yl)
    if not loo:
        mode = weight_mode(wu, unbiased, K)
        W, mag = weight(PS, K, mode, wu)
        want = Yl * W[None, :]
        bound = None if mode == 2 else (NOPS[mode] + 1) * EPS * mag[None, :] * aY
        return FilterRef(want, bound, W, mode, K)
    assert K >= 2
    K1 = K - 1
    mode = weight_mode(wu, unbiased, K1)
    q = np.asarray(PS).astype(CLD)[None, :] - phasors(Y)
    W, mag = weight(q, K1, mode, wu)
    want = Yl * W
    bound = None
    if mode != 2:
        r = np.abs(q)
        dq = PHASOR + EPS * r
        bound = ((NOPS[mode] + 1) * EPS * mag + _dW(r, K1, mode, wu) * dq + (dq / LD(K1)) ** 2) * aY
    return FilterRef(want, bound, W, mode, K1)


class FilterMismatch(AssertionError):
    """A coefficient outside its bound: .row, .index, .ratio."""

    def __init__(self, msg, row, index, ratio):
        super().__init__(msg)
        self.row, self.index, self.ratio = row, index, ratio


def check_sets(got, ref, what=""):
    """|got - want| <= bound at EVERY coefficient of every row (NaN fails); mode 2: max |got - want| <= PARITY max |want| per row.  Returns
    the worst ratio."""
    got = np.asarray(got)
    assert got.shape == ref.want.shape and got.dtype == np.complex128, (got.shape, ref.want.shape, got.dtype)
    diff = np.abs(got.astype(CLD) - ref.want)
    if ref.bound is None:
        lim = LD(PARITY) * np.abs(ref.want).max(axis=1)
        worst = diff.max(axis=1)
        bad = ~(worst <= lim) | ~np.isfinite(got).all(axis=1)
        ratio = np.where(lim > 0, worst / np.where(lim > 0, lim, 1), np.where(worst > 0, np.inf, 0)).astype(np.float64)
        if bad.any():
            i = int(np.argmax(np.where(bad, ratio, -1)))
            raise FilterMismatch(f"{what}: row {i} of {len(got)} (mode 2) outside the parity tolerance: max |diff| / (2e-6 max |want|) = {ratio[i]:.3g}", i, -1,
                                 float(ratio[i]))
        return float(ratio.max()) if ratio.size else 0.0
    bound = ref.bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0))
    ratio = np.where(np.isfinite(got), ratio, np.inf).astype(np.float64)
    if not ratio.size:
        return 0.0
    i, k = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    nbad = int(np.count_nonzero(~(ratio <= 1.0)))
    if nbad:
        raise FilterMismatch(f"{what}: {nbad} coefficient(s) outside the bound (mode {ref.mode}, K = {ref.K}); worst in row {i}, coefficient {k}: got "
                             f"{complex(got[i, k])!r}, want {complex(ref.want[i, k])!r}, |diff| / bound = {ratio[i, k]:.3g} (bound {float(bound[i, k]):.3g})",
                             i, k, float(ratio[i, k]))
    return float(ratio[i, k])


def rows_of(fr, Yw):
    """The real rows [R][N] (longdouble) of the coefficient sets Yw[R][ncoef] (any complex type), scale by scale through
    inverse_rows_ref.scale_rows, added in increasing s."""
    Yw = np.asarray(Yw)
    x = np.zeros((Yw.shape[0], fr.N), LD)
    if not Yw.shape[0]:
        return x
    with ThreadPoolExecutor(irr._workers()) as pool:       # (numpy releases the GIL inside the long array operations; added in scale order)
        for xs in pool.map(lambda s: irr.scale_rows(fr, s, Yw[:, fr.off[s]: fr.off[s + 1]])[0], range(fr.S)):
            x += xs
    return x


def filtered_rows(fr, Y, PS, K, wu, unbiased, loo=False):
    """x~[M][N] (longdouble) of one ensemble's sets: the rows of reference(...).want."""
    return rows_of(fr, reference(Y, np.asarray(PS).astype(np.complex128), K, wu, unbiased, loo).want)


def group_sums(Y, Kmax):
    """The sets of the Kmax partial stacks of a two-stage ensemble, by linearity: group g = the traces i with floor(i Kmax / M) == g
    (partial_linear_stacks, ts_pws1f_lib.c:866-881)."""
    Y = np.asarray(Y)
    M = len(Y)
    g = (np.arange(M, dtype=np.int64) * Kmax) // M
    out = np.zeros((Kmax, Y.shape[1]), CLD)
    for i in range(M):
        out[g[i]] += Y[i].astype(CLD)
    return out
