"""The checker of the wavelet cross-spectrum calls (tspws_hip_wxs_coef / tspws_hip_wxs_rows): from two coefficient sets it evaluates the
contract's definition in np.longdouble -- the cross-spectrum X = c conj(r), a = |X|, phi = arg X, delta = phi / omega_s, t = k D_s - z and the
nine sums per (row, window, band) -- and beside every sum a bound that a correct FP64 implementation stays inside WHATEVER the order of its
operations, fused or not.  No GPU import here.

What is shared with the device exactly: the FP64 bits of the coefficients, z, and omega_s = w0 / scale_s formed by ONE FP64 division (as the
library forms it on the host).  With u = 2**-53, per coefficient:

  xr, xi   two products and one addition each: |xr - xr*| <= b_xr = 2.01 u (|c.re r.re| + |c.im r.im|), b_xi likewise
  a        hypot is accurate to H ulp, and one ulp of a is at most 2 u a: b_a = (b_xr + b_xi) + 2.01 H u (a* + b_xr + b_xi)
           (|hypot(x + e) - hypot(x)| <= |e| <= b_xr + b_xi)
  phi      atan2 is accurate to T ulp: b_phi = 1.6 (b_xr + b_xi) / a* + 2.01 T u (|phi*| + ...) -- moving the point by e turns it by at most
           asin(e / a*) <= 1.6 e / a* while e <= a* / 2; beyond that b_phi = 2 pi (no two values of atan2 differ by more).
           A FLIP term: Re X* < 0 and |Im X*| <= b_xi with b_xi > 0 -- FP64 rounding cannot decide the sign of Im X, the phase may come out
           at +pi or at -pi -- gets 2 pi added to b_phi, which the products below carry into Ad, Atd and Add (2 pi a / omega_s in Ad); these
           terms are counted (`flips`), and the parity inputs are chosen so that there are none.
  delta    one division: b_delta = 1.01 (b_phi / omega + u |delta*|)
  t        (double)(k D) is exact, the subtraction rounds once: b_t = u |t*|
  a term   a product of m factors x_j known to b_j, formed with m - 1 roundings in any association:
           b = prod (|x_j| + b_j) - prod |x_j| + 1.01 (m - 1) u prod (|x_j| + b_j)
  a sum    n terms added in any order, each addition rounded: b = sum b_term + 1.01 (n - 1) u sum (|term*| + b_term)

H and T: the ROCm installation ships no accuracy table for its device library's double-precision hypot and atan2, so the OpenCL full-profile
limits are used: hypot <= 4 ulp, atan2 <= 6 ulp.

Participation must be decided by the inputs: a term whose a* is not zero but within b_a of zero (or not finite) is counted in `undecided`,
and the tests assert that there is none; then n is exact.  The longdouble evaluation itself errs by about 2**-64 per operation, two thousand
times below the bounds.  No tolerance is fitted to an output."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
H_ULP, T_ULP = 4, 6   # OpenCL full profile, double: hypot, atan2
N, Z = 1501, 750.0
NAMES = ("n", "A", "At", "Att", "Ad", "Atd", "Add", "Xr", "Xi")


class Frame:
    """What the checker needs of a frame: N, w0 and the per-scale tables (scale, D, Ns, c, L) -- a Plan's (tables(), info.w0) or the
    oracle's (abi.OracleFrame: the same tables)."""

    def __init__(self, N, w0, scale, D, Ns, c, L):
        self.N, self.w0 = int(N), np.float64(w0)
        self.scale = np.asarray(scale, np.float64)
        self.D, self.Ns, self.c, self.L = (np.asarray(a).astype(np.int64) for a in (D, Ns, c, L))
        self.S = len(self.D)
        self.off = np.concatenate([[0], np.cumsum(self.Ns)]).astype(np.int64)
        self.ncoef = int(self.off[-1])
        self.omega = self.w0 / self.scale  # ONE FP64 division per scale

    @classmethod
    def from_plan(cls, pl):
        t = pl.tables()
        return cls(pl.N, pl.info.w0, t["scale"], t["D"], t["Ns"], t["c"], t["L"])

    @classmethod
    def from_oracle(cls, p, N):
        """Of the RESOLVED parameter set p; .oracle keeps the oracle's frame (its forward transform is the CPU tests' source of sets)."""
        import abi
        f = abi.OracleFrame.from_params(p, N)
        fr = cls(N, p.w0, f.scale, f.D, f.Ns, f.c, f.L)
        fr.oracle = f
        return fr

    def octave_bands(self):
        """The frame's decimation octaves as bands: runs of scales with one D."""
        edges = [0] + [s for s in range(1, self.S) if self.D[s] != self.D[s - 1]] + [self.S]
        return [(a, b) for a, b in zip(edges[:-1], edges[1:])]


def members(fr, s, win, skip_wrapped):
    """The indices k of scale s whose sample k D lies in the window and, under the wrap rule, whose filter support lies inside [0, N)."""
    k = np.arange(fr.Ns[s], dtype=np.int64)
    at = k * fr.D[s]
    ok = (at >= win[0]) & (at < win[1])
    if skip_wrapped:
        ok &= (at - fr.c[s] >= 0) & (at - fr.c[s] + fr.L[s] <= fr.N)
    return k[ok]


def _term(*factors):
    """(value, bound) of a product of (x*, b) factors formed with len - 1 roundings."""
    val, hi = LD(1), LD(1)
    for x, b in factors:
        val = val * x
        hi = hi * (np.abs(x) + b)
    return val, hi - np.abs(val) + LD(1.01) * (len(factors) - 1) * LD(U) * hi


def scale_terms(fr, s, k, c, r, z):
    """The nine terms of the coefficients k of scale s (c, r: complex128 arrays over k): dict of values [9][len k] and bounds (longdouble),
    `part` (bool: the coefficient takes part), and the counts of flip and undecided terms."""
    cr, ci, rr, ri = (np.asarray(v, np.float64).astype(LD) for v in (c.real, c.imag, r.real, r.imag))
    u = LD(U)
    xr, xi = cr * rr + ci * ri, ci * rr - cr * ri
    bxr, bxi = LD(2.01) * u * (np.abs(cr * rr) + np.abs(ci * ri)), LD(2.01) * u * (np.abs(ci * rr) + np.abs(cr * ri))
    e = bxr + bxi
    a = np.hypot(xr, xi)
    finite = np.isfinite(a.astype(np.float64)) & np.isfinite(np.asarray(c)) & np.isfinite(np.asarray(r))
    ba = e + LD(2.01) * H_ULP * u * (a + e)
    part = finite & (a > 0)
    undecided = int((~finite | ((a > 0) & (a <= ba))).sum())
    safe = np.where(part, a, LD(1))
    phi = np.arctan2(xi, xr)
    flip = part & (xr < 0) & (np.abs(xi) <= bxi) & (bxi > 0)
    bphi = np.where(e <= safe / 2, LD(1.6) * e / safe, 2 * LD(np.pi)) + LD(2.01) * T_ULP * u * (np.abs(phi) + LD(1.6) * e / safe)
    bphi = np.minimum(bphi, 2 * LD(np.pi)) + np.where(flip, 2 * LD(np.pi), 0)
    om = LD(fr.omega[s])
    delta = phi / om
    bdelta = LD(1.01) * (bphi / om + u * np.abs(delta))
    t = (k * fr.D[s]).astype(LD) - LD(np.float64(z))
    bt = u * np.abs(t)
    one = np.ones_like(a)
    A, T, Dl = (a, ba), (t, bt), (delta, bdelta)
    terms = [(one, 0 * one), A, _term(A, T), _term(A, T, T), _term(A, Dl), _term(A, T, Dl), _term(A, Dl, Dl), (xr, bxr), (xi, bxi)]
    val = np.stack([np.where(part, v, 0) for v, _ in terms])
    bnd = np.stack([np.where(part, b, 0) for _, b in terms])
    return dict(val=val, bnd=bnd, part=part, flips=int(flip.sum()), undecided=undecided)


def reference(fr, Yc, Yr, z, bands, windows, ens=None, skip_wrapped=False, take=None):
    """dict for the sets Yc [nrow][ncoef] against Yr [B][ncoef] (complex128): sums and b_sums (longdouble [nrow][W][R][9]; NaN for the rows
    with take[i] false), flips and undecided (counts over all terms).  A scale's terms are formed once per (row, window) and shared by the
    bands that hold it."""
    nrow, W, R = Yc.shape[0], len(windows), len(bands)
    sums = np.zeros((nrow, W, R, 9), LD)
    absb = np.zeros((nrow, W, R, 9), LD)  # sum of |term*| + b_term
    bsum = np.zeros((nrow, W, R, 9), LD)  # sum of b_term
    used = sorted({s for a, b in bands for s in range(a, b)})
    flips = undecided = 0
    for i in range(nrow):
        if take is not None and not take[i]:
            sums[i] = np.nan
            continue
        b = i if ens is None else int(ens[i])
        for w, win in enumerate(windows):
            for s in used:
                k = members(fr, s, win, skip_wrapped)
                if not k.size:
                    continue
                o = fr.off[s]
                tm = scale_terms(fr, s, k, Yc[i, o + k], Yr[b, o + k], z)
                flips += tm["flips"]
                undecided += tm["undecided"]
                v, bb, ab = tm["val"].sum(axis=1), tm["bnd"].sum(axis=1), (np.abs(tm["val"]) + tm["bnd"]).sum(axis=1)
                for r_, (s0, s1) in enumerate(bands):
                    if s0 <= s < s1:
                        sums[i, w, r_] += v
                        bsum[i, w, r_] += bb
                        absb[i, w, r_] += ab
    n = np.maximum(sums[..., :1], 1)
    b_sums = bsum + LD(1.01) * (n - 1) * LD(U) * absb
    b_sums[..., 0] = 0
    b_sums[np.isnan(sums)] = np.nan
    return dict(sums=sums, b_sums=b_sums, flips=flips, undecided=undecided)


def check(sums, want, what=""):
    """Every entry of the float64 `sums` [..][9] inside its bound, n exact, NaN exactly where the checker has NaN.  Prints the largest
    |error| / bound per sum before it asserts; returns those nine ratios."""
    sums = np.asarray(sums)
    ref, b = want["sums"].reshape(sums.shape), want["b_sums"].reshape(sums.shape)
    nan = np.isnan(ref.astype(np.float64))
    assert np.array_equal(np.isnan(sums), nan), f"{what}: NaN positions of the sums differ"
    assert want["undecided"] == 0, f"{what}: {want['undecided']} terms whose participation the inputs do not decide"
    live = ~nan[..., 0]
    err = np.abs(sums[live].astype(LD) - ref[live])
    bb = b[live]
    assert np.isfinite(bb.astype(np.float64)).all(), f"{what}: an infinite bound"
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(err == 0, 0, err / bb).astype(np.float64)  # (an error against a zero bound: inf)
    worst = frac.reshape(-1, 9).max(axis=0) if frac.size else np.zeros(9)
    print(what, "worst |error| / bound:", " ".join(f"{n} {v:.3g}" for n, v in zip(NAMES, worst)), f"; flips {want['flips']}")
    assert np.array_equal(sums[live][..., 0], ref[live][..., 0].astype(np.float64)), f"{what}: n differs"
    assert (worst <= 1).all(), f"{what}: a sum outside its bound ({dict(zip(NAMES, worst))})"
    return worst


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------
def cr_hypot(x, y):
    """The correctly rounded hypot of two finite float64, by exact rational comparison against the neighbours' midpoints."""
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y)):
        return math.hypot(x, y)
    s = Fraction(x) ** 2 + Fraction(y) ** 2
    if s == 0:
        return 0.0
    h = math.hypot(x, y)
    while Fraction(h) ** 2 > s and ((Fraction(h) + Fraction(math.nextafter(h, 0.0))) / 2) ** 2 > s:
        h = math.nextafter(h, 0.0)
    while Fraction(h) ** 2 < s and ((Fraction(h) + Fraction(math.nextafter(h, math.inf))) / 2) ** 2 < s:
        h = math.nextafter(h, math.inf)
    return h


def fit(sums):
    """The contract's fit in numpy float64, every operation rounded on its own, on a float64 sums array [..][9]: [..][6] = eps_hat, icpt,
    err, rms, coh, n.  NaN sums (a row left out) give five NaN and n = -1."""
    sums = np.asarray(sums, np.float64)
    out = np.empty(sums.shape[:-1] + (6,), np.float64)
    nan = np.float64("nan")
    for idx in np.ndindex(*sums.shape[:-1]):
        n, A, At, Att, Ad, Atd, Add, Xr, Xi = (np.float64(v) for v in sums[idx])
        if np.isnan(n):
            out[idx] = (nan, nan, nan, nan, nan, -1.0)
            continue
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            coh = np.float64(cr_hypot(Xr, Xi)) / A
            den = A * Att - At * At
            if n >= 2 and den > 0:
                eh = (A * Atd - At * Ad) / den
                ic = (Att * Ad - At * Atd) / den
                res = (Add - ic * Ad) - eh * Atd
                rms = np.sqrt((res if res > 0 else np.float64(0)) / A)
                out[idx] = (eh, ic, rms * np.sqrt(A / den), rms, coh, n)
            else:
                out[idx] = (nan, nan, nan, nan, coh, n)
    return out


# ---- a plain FP64 evaluation in several orders (the checker's own test) -----------------------------------------------------------------
def _sum(v, order):
    if order == "pairwise":
        while v.shape[-1] > 1:
            if v.shape[-1] % 2:
                v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], axis=-1)
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0] if v.shape[-1] else np.zeros(v.shape[:-1])
    if order == "reversed":
        v = v[..., ::-1]
    return np.cumsum(v, axis=-1)[..., -1] if v.shape[-1] else np.zeros(v.shape[:-1])


def fp64_sums(fr, yc, yr, z, bands, windows, skip_wrapped=False, order="forward", wrong=None):
    """sums float64 [W][R][9] of ONE pair of sets, every operation in numpy FP64, the terms of a (window, band) gathered over its scales and
    added in `order`; "reversed" also associates the triple products the other way.  wrong=(s, j): the phase of the j-th member of scale s
    is taken with the opposite sign (a deliberately wrong term)."""
    out = np.zeros((len(windows), len(bands), 9))
    for w, win in enumerate(windows):
        for r_, (s0, s1) in enumerate(bands):
            cols = []
            for s in range(s0, s1):
                k = members(fr, s, win, skip_wrapped)
                c, r = yc[fr.off[s] + k], yr[fr.off[s] + k]
                xr, xi = c.real * r.real + c.imag * r.imag, c.imag * r.real - c.real * r.imag
                a = np.hypot(xr, xi)
                phi = np.arctan2(xi, xr)
                if wrong is not None and wrong[0] == s and k.size:
                    phi[wrong[1] % k.size] *= -1
                delta = phi / fr.omega[s]
                t = (k * fr.D[s]).astype(np.float64) - np.float64(z)
                if order == "reversed":
                    rows = [np.ones_like(a), a, t * a, (t * t) * a, delta * a, (t * delta) * a, (delta * delta) * a, xr, xi]
                else:
                    rows = [np.ones_like(a), a, a * t, a * t * t, a * delta, a * t * delta, a * delta * delta, xr, xi]
                ok = np.isfinite(a) & (a > 0)
                cols.append(np.stack(rows)[:, ok])
            if cols:
                out[w, r_] = _sum(np.concatenate(cols, axis=1), order)
    return out


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------------
WINDOWS = ((3, 611), (890, 1501), (0, 1501))   # edges that are no multiples of any D; the last touches both trace ends
ZS = (750.0, 0.0, 750.25)


def parity_bands(fr):
    """R = 5: one octave, one cut between voices, two overlapping, one empty."""
    oc = fr.octave_bands()
    assert len(oc) >= 4 and oc[1][1] - oc[1][0] >= 2
    return [oc[1], (oc[1][0] + 1, oc[2][0] + 1), (oc[0][0], oc[2][1]), (oc[1][0], oc[3][1]), (oc[2][0], oc[2][0])]


def parity_batch(seed, B=3, M=9):
    """(rows float32 [B][M][N + 3], ref float32 [B][N + 1], counts uint32 [B][M]) with NaN pad columns: ensemble b has its own wavelet
    (stretch_rows_ref.wavelet); row m is the analytically stretched wavelet plus seeded noise of sigma 0, 0.2 or 1 (m % 3), scaled by
    1e-6 .. 1e2; row (0, 5) is all zero; the reference of ensemble 1 is zero inside [3, 611); the counts leave out 0 / 4 / 8 rows."""
    import stretch_rows_ref as srr
    rng = np.random.default_rng(seed)
    rows = np.full((B, M, N + 3), np.nan, np.float32)
    ref = np.full((B, N + 1), np.nan, np.float32)
    t = np.arange(N, dtype=np.float64) - Z
    eps0 = (0.0037, -0.00612, 0.0, 0.0081, -0.0029, 0.0011, -0.0093)
    for b in range(B):
        a = srr.wavelet(1000 * seed + b)
        ref[b, :N] = a(t)
        for m in range(M):
            x = a(t * (1 + eps0[m % len(eps0)])) + (0.0, 0.2, 1.0)[m % 3] * rng.standard_normal(N)
            rows[b, m, :N] = x * 10.0 ** rng.uniform(-6, 2)
    rows[0, 5, :N] = 0
    if B > 1:
        ref[1, 3:611] = 0
    mtr = np.full((B, M), 7, np.uint32)
    if B > 2:
        mtr[1, 1:8:2] = 0    # 4 rows left out
        mtr[2] = 0
        mtr[2, 6] = 3        # one row takes part
    return rows, ref, mtr


# recovery: a band-limited decaying coda at N = 4096 and its copy at lag t (1 + eps), by sinc interpolation in float64
RN, RZ, REPS = 4096, 2048.0, 2e-3
RWIN = ((2148, 2548),)   # 100 .. 500 samples of lag: |omega eps t| <= 2 pi 0.13 * 2e-3 * 500 = 0.82 < pi / 2 for every scale of the band


def recovery_rows(seed=0):
    """(ref float32 [RN], row float32 [RN]): white noise under the envelope exp(-|t| / 600), band-passed to 0.04 .. 0.16 cycles per sample,
    and row(t) = ref(t (1 + REPS)) by sinc interpolation of the float64 reference (band-limited: the interpolation is exact up to its
    truncation at the trace ends, far from the window)."""
    rng = np.random.default_rng(seed)
    t = np.arange(RN, dtype=np.float64) - RZ
    X = np.fft.rfft(rng.standard_normal(RN) * np.exp(-np.abs(t) / 600))
    f = np.fft.rfftfreq(RN)
    X *= np.exp(-0.5 * ((f - 0.10) / 0.02) ** 2) * ((f > 0.04) & (f < 0.16))
    x = np.fft.irfft(X, RN)
    x = x / np.abs(x).max()
    u = RZ + t * (1 + REPS)                                   # where the row looks at the reference, in samples
    row = (np.sinc(u[:, None] - np.arange(RN)[None, :]) * x[None, :]).sum(axis=1)
    return x.astype(np.float32), row.astype(np.float32)


def recovery_band(fr):
    """The scales whose centre frequency omega / 2 pi lies in [0.07, 0.13) cycles per sample."""
    fc = fr.omega / (2 * np.pi)
    s = np.nonzero((fc >= 0.07) & (fc < 0.13))[0]
    assert s.size and (np.diff(s) == 1).all()
    return [(int(s[0]), int(s[-1]) + 1)]
