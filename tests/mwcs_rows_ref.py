"""The checker of tspws_hip_mwcs_rows: a np.longdouble evaluation of the contract (include/tspws_hip.h) and, beside every value, a bound
that a correct FP64 implementation stays inside.  No GPU import here.

STAGE 1 (any order of FP64 evaluation).  The ideal table g*, C*, S* is evaluated in longdouble; the device's table holds every entry
rounded once.  With u = 2**-53, for one window x[0 .. L) and one column c* of the table (T* = sum_l c*[l]):
  dot    sum_l x[l] c[l], L products and L - 1 additions in any order and any fusion, on entries c[l] = c*[l] (1 + d), |d| <= 1.01 u:
         b_dot = 1.01 u S1 + 1.01 (L + 1) u S1 with S1 = sum |x c*|
  mu     L - 1 additions in any order and one division: b_mu = 1.01 L u (sum |x|) / L
  T      the rounded entries added in ascending l: b_T = 1.01 u sum |c*| + 1.01 (L - 1) u sum |c*|
  mu T   one product: b_mT = (|mu*| + b_mu)(|T*| + b_T) - |mu* T*| + 1.01 u (|mu*| + b_mu)(|T*| + b_T)
  F      one subtraction: b_F = b_dot + b_mT + 1.01 u (|dot*| + b_dot + |mu* T*| + b_mT)
STAGES 2 AND 3 are evaluated from the DEVICE's stage-1 bits (exact inputs) with the table's k and v as the library's host function returns
them (shared exactly).  Every value carries a bound through every operation:
  product  b = (|x| + bx)(|y| + by) - |x y| + 1.01 u (|x| + bx)(|y| + by)
  sum      (any association) b = sum b_i + 1.01 (n - 1) u sum (|x_i| + b_i)
  quotient (|y| > by) b = (|x| + bx) / (|y| - by) - |x / y| + 1.01 u (|x| + bx) / (|y| - by)
  sqrt     b = max(sqrt(x + bx) - sqrt(x), sqrt(x) - sqrt(max(x - bx, 0))) + 1.01 u sqrt(x + bx)
  hypot, atan2  as tests/wxs_rows_ref.py: the OpenCL full-profile limits (4 and 6 ulp; the ROCm installation states none) on top of the
           propagated input error e: b_a = e + 2.01 H u (a + e); b_phi = 1.6 e / a + 2.01 T u (|phi| + 1.6 e / a) while e <= a / 2, else 2 pi
  min(coh, 0.99)  is 1-Lipschitz: the bound passes through
Terms whose outcome FP64 rounding could flip are COUNTED (`undecided`), and the tests take inputs that have none: a phase at +-pi (Re X < 0
and |Im X| within its bound), coh within its bound of the 0.99 clip, a filter of stage 3 within the bound of its threshold (or a window
whose finiteness is not decided), smPc smPr within its bound of zero but not zero.
The longdouble evaluation itself errs by about 2**-64 per operation, two thousand times below the bounds.  No tolerance is fitted to an
output."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
u = LD(U)
K = LD(1.01)
H_ULP, T_ULP = 4, 6   # OpenCL full profile, double: hypot, atan2
N, Z = 1501, 750.0
ZS = (750.0, 0.0, 750.25)
PI = LD("3.14159265358979323846264338327950288")


class Par:
    """The parameters, as tspws_mwcs_par holds them."""

    def __init__(self, L, hop, P, q0, q1, h=0, taper=0.0, min_coh=0.0, max_err=float("inf"), max_delta=float("inf"), err_floor=1e-6):
        self.L, self.hop, self.P, self.q0, self.q1, self.h = L, hop, P, q0, q1, h
        self.taper, self.min_coh, self.max_err, self.max_delta, self.err_floor = (np.float64(v) for v in (taper, min_coh, max_err, max_delta, err_floor))
        self.qa, self.qb = max(0, q0 - h), min(P // 2 + 1, q1 + h)
        self.Qx, self.nq = self.qb - self.qa, q1 - q0

    def kwargs(self):
        return dict(L=self.L, hop=self.hop, P=self.P, q0=self.q0, q1=self.q1, h=self.h, taper=float(self.taper), min_coh=float(self.min_coh),
                    max_err=float(self.max_err), max_delta=float(self.max_delta), err_floor=float(self.err_floor))


def windows(par, ranges):
    """[(n_j, w)] by the definition: range w = [n0, n1) holds the windows n0 + j hop, j < J_w = (n1 - n0 - L) // hop + 1 when n1 - n0 >= L."""
    out = []
    for w, (n0, n1) in enumerate(ranges):
        Jw = (n1 - n0 - par.L) // par.hop + 1 if n1 - n0 >= par.L else 0
        out += [(n0 + j * par.hop, w) for j in range(Jw)]
    return out


def basis(par):
    """The ideal table in longdouble: dict g [L], C, S [L][Qx], Tc, Ts [Qx] (exact sums of the ideal entries, in longdouble)."""
    L, P = par.L, par.P
    l = np.arange(L)
    a = np.float64(par.taper) * np.float64(L) * np.float64(0.5)
    x = np.minimum(l + 0.5, (L - 0.5) - l)
    g = np.where(x < a, LD(0.5) * (1 - np.cos(PI * x.astype(LD) / LD(a if a > 0 else 1))), LD(1))
    m = (np.arange(par.qa, par.qb)[None, :] * l[:, None]) % P
    ang = 2 * PI * m.astype(LD) / LD(P)
    return dict(g=g, ang=ang)


def ideal_table(par, g64):
    """C*, S* in longdouble from the ROUNDED taper g64 (the contract: C = g[l] cos(..), one rounding per entry) [L][Qx]."""
    ang = basis(par)["ang"]
    gl = np.asarray(g64, np.float64).astype(LD)[:, None]
    return gl * np.cos(ang), -(gl * np.sin(ang))


def ulps(got, want):
    """|got - want| in units of the spacing of float64 at want (longdouble `want`)."""
    w64 = np.abs(want.astype(np.float64))
    sp = np.spacing(np.where(w64 > 0, w64, np.float64(1e-300)))
    return (np.abs(got.astype(LD) - want) / sp.astype(LD)).astype(np.float64)


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------------
def frames(x, par, wins):
    """float32 [..][>= N] -> longdouble windows [..][J][L]."""
    idx = np.array([n for n, _ in wins], dtype=np.int64)[:, None] + np.arange(par.L)[None, :]
    return np.asarray(x)[..., idx].astype(np.float64).astype(LD)


def stage1(x, par, wins, g64):
    """(F* complex as (re, im) longdouble [..][J][Qx], b_re, b_im) of float32 rows x [..][>= N]."""
    X = frames(x, par, wins)
    L = par.L
    Cs, Ss = ideal_table(par, g64)
    sabs = np.abs(X).sum(axis=-1, keepdims=True)
    mu = X.sum(axis=-1, keepdims=True) / L
    b_mu = K * L * u * sabs / L
    out = []
    for tab in (Cs, Ss):
        dot = X @ tab
        S1 = np.abs(X) @ np.abs(tab)
        b_dot = K * u * S1 + K * (L + 1) * u * S1
        T = tab.sum(axis=0)
        b_T = K * u * np.abs(tab).sum(axis=0) + K * (L - 1) * u * np.abs(tab).sum(axis=0)
        hi = (np.abs(mu) + b_mu) * (np.abs(T) + b_T)
        b_mT = hi - np.abs(mu * T) + K * u * hi
        F = dot - mu * T
        out.append((F, b_dot + b_mT + K * u * (np.abs(dot) + b_dot + np.abs(mu * T) + b_mT)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def fp64_stage1(x, par, wins, g64):
    """An independent plain-numpy FP64 evaluation through numpy.fft.rfft: complex128 [..][J][Qx] of the demeaned, tapered, zero-padded windows."""
    idx = np.array([n for n, _ in wins], dtype=np.int64)[:, None] + np.arange(par.L)[None, :]
    X = np.asarray(x)[..., idx].astype(np.float64)
    X = (X - X.mean(axis=-1, keepdims=True)) * np.asarray(g64, np.float64)
    return np.fft.rfft(X, n=par.P, axis=-1)[..., par.qa:par.qb]


# ---- bound arithmetic ------------------------------------------------------------------------------------------------------------------
def mul(a, b):
    (x, bx), (y, by) = a, b
    hi = (np.abs(x) + bx) * (np.abs(y) + by)
    return x * y, hi - np.abs(x * y) + K * u * hi


def add(*terms):
    val = sum(t[0] for t in terms)
    return val, sum(t[1] for t in terms) + K * (len(terms) - 1) * u * sum(np.abs(t[0]) + t[1] for t in terms)


def vsum(t, axis=-1):
    """The sum of an array of terms along an axis, any association."""
    x, b = t
    n = x.shape[axis]
    return x.sum(axis=axis), b.sum(axis=axis) + K * max(n - 1, 0) * u * (np.abs(x) + b).sum(axis=axis)


def div(a, b):
    (x, bx), (y, by) = a, b
    with np.errstate(invalid="ignore", divide="ignore"):
        lo = np.abs(y) - by
        hi = np.where(lo > 0, (np.abs(x) + bx) / np.where(lo > 0, lo, 1), np.inf)
        q = x / y
        return q, hi - np.abs(q) + K * u * hi


def sqrt(a):
    x, bx = a
    with np.errstate(invalid="ignore"):
        s, hi, lo = np.sqrt(x), np.sqrt(x + bx), np.sqrt(np.maximum(x - bx, 0))
        return s, np.maximum(hi - s, s - lo) + K * u * hi


def neg(a):
    return -a[0], a[1]


def exact(x):
    x = np.asarray(x, np.float64).astype(LD)
    return x, np.zeros_like(x)


# ---- stages 2 and 3 --------------------------------------------------------------------------------------------------------------------
def stage2(Fc, Fr, par, tab):
    """From complex128 device spectra Fc [..][J][Qx] and Fr (broadcastable): dict delta, err, mcoh (longdouble [..][J]) with bounds b_*, `nan`
    (bool: smPc smPr == 0 in a bin of the band) and the count `undecided`."""
    cr, ci, rr, ri = exact(Fc.real), exact(Fc.imag), exact(np.broadcast_to(Fr, Fc.shape).real), exact(np.broadcast_to(Fr, Fc.shape).imag)
    planes = [add(mul(cr, rr), mul(ci, ri)), add(mul(ci, rr), neg(mul(cr, ri))), add(mul(cr, cr), mul(ci, ci)), add(mul(rr, rr), mul(ri, ri))]
    h, lo, nq, Qx = par.h, par.q0 - par.qa, par.nq, par.Qx
    kk = exact(tab["k"])
    sm = []
    for x, b in planes:
        cols = []
        for q in range(lo, lo + nq):
            ds = [d for d in range(-h, h + 1) if 0 <= q + d < Qx]
            num = add(*[mul((kk[0][d + h], kk[1][d + h]), (x[..., q + d], b[..., q + d])) for d in ds])
            ks = add(*[(kk[0][d + h], kk[1][d + h]) for d in ds])
            cols.append(div(num, (np.broadcast_to(ks[0], num[0].shape), np.broadcast_to(ks[1], num[0].shape))))
        sm.append((np.stack([c[0] for c in cols], axis=-1), np.stack([c[1] for c in cols], axis=-1)))
    sxr, sxi, spc, spr = sm
    e = sxr[1] + sxi[1]
    a = np.hypot(sxr[0], sxi[0])
    ba = e + LD(2.01) * H_ULP * u * (a + e)
    pp = mul(spc, spr)
    nan = (pp[0] == 0).any(axis=-1)
    und = int(((pp[0] != 0) & (np.abs(pp[0]) <= pp[1])).sum())
    live = ~nan[..., None] & np.ones(a.shape, bool)
    safe_a = np.where(a > 0, a, LD(1))
    phi = np.arctan2(sxi[0], sxr[0])
    turn = LD(1.6) * e / safe_a
    bphi = np.where((e <= a / 2) & (a > 0), turn + LD(2.01) * T_ULP * u * (np.abs(phi) + turn), 2 * PI)
    flip = live & (sxr[0] < 0) & (np.abs(sxi[0]) <= sxi[1])
    und += int(flip.sum())
    bphi = bphi + np.where(flip, 2 * PI, 0)
    pp_s = (np.where(live, pp[0], LD(1)), np.where(live, pp[1], LD(0)))
    coh = div((a, ba), sqrt(pp_s))
    und += int((live & (np.abs(coh[0] - LD(np.float64(0.99))) <= coh[1])).sum())
    cc = (np.minimum(coh[0], LD(np.float64(0.99))), coh[1])
    c2 = mul(cc, cc)
    one = exact(np.ones(a.shape))
    wq = sqrt(mul(div(c2, add(one, neg(c2))), sqrt((a, ba))))
    v = exact(np.broadcast_to(np.asarray(tab["v"], np.float64)[lo:lo + nq], a.shape))
    wv = mul(wq, v)
    Svv, Svp, Sw2, Sc = vsum(mul(wv, v)), vsum(mul(wv, (phi, bphi))), vsum(mul(wv, wv)), vsum(coh)
    delta = div(Svp, Svv)
    res = add((phi, bphi), neg(mul((delta[0][..., None], delta[1][..., None]), v)))
    s2 = div(vsum(mul(res, res)), exact(np.full(delta[0].shape, nq - 1.0)))
    err = div(sqrt(mul(Sw2, s2)), Svv)
    mcoh = div(Sc, exact(np.full(delta[0].shape, float(nq))))
    out = {}
    for name, (x, b) in (("delta", delta), ("err", err), ("mcoh", mcoh)):
        out[name] = np.where(nan, LD("nan"), x)
        out["b_" + name] = np.where(nan, LD("nan"), b)
    out["nan"], out["undecided"] = nan, und
    return out


def takes_part(s2, par):
    """(take bool [..][J], undecided count) of the filters of stage 3 on the checker's stage 2."""
    d, e, c = s2["delta"], s2["err"], s2["mcoh"]
    bd, be, bc = s2["b_delta"], s2["b_err"], s2["b_mcoh"]
    with np.errstate(invalid="ignore"):
        fin = ~s2["nan"] & np.isfinite(d.astype(np.float64)) & np.isfinite(e.astype(np.float64)) & np.isfinite(bd.astype(np.float64)) & np.isfinite(be.astype(np.float64))
        und = int((~s2["nan"] & ~fin).sum())
        take = fin & (e <= LD(par.max_err)) & (c >= LD(par.min_coh)) & (np.abs(d) <= LD(par.max_delta))
        for x, b, thr in ((e, be, par.max_err), (c, bc, par.min_coh), (np.abs(d), bd, par.max_delta)):
            if np.isfinite(thr):
                und += int((fin & (np.abs(x - LD(thr)) <= b)).sum())
    return take, und


def fit(win, par, wins, W, z):
    """The contract's stage 3 in numpy float64, every operation rounded on its own, on a float64 d_win [..][J][3]: [..][W][6].  A row
    whose windows are all NaN AND whose `left_out` flag is set is the caller's to overwrite (see fit_rows)."""
    win = np.asarray(win, np.float64)
    lead = win.shape[:-2]
    out = np.full(lead + (W, 6), np.nan)
    L = np.float64(par.L)
    with np.errstate(all="ignore"):
        for w in range(W):
            S, St, Stt, Sd, Std, n = (np.zeros(lead) for _ in range(6))
            for j, (n0, ww) in enumerate(wins):
                if ww != w:
                    continue
                d, e, c = win[..., j, 0], win[..., j, 1], win[..., j, 2]
                t = (np.float64(n0) + np.float64(0.5) * (L - np.float64(1))) - np.float64(z)
                take = np.isfinite(d) & np.isfinite(e) & (e <= par.max_err) & (c >= par.min_coh) & (np.abs(d) <= par.max_delta)
                ee = np.where(e > par.err_floor, e, par.err_floor)
                p = np.float64(1) / (ee * ee)
                pt = p * t
                S, St, Stt, Sd, Std, n = (np.where(take, acc + v, acc) for acc, v in ((S, p), (St, pt), (Stt, pt * t), (Sd, p * d), (Std, pt * d), (n, 1.0)))
            den = S * Stt - St * St
            ok = (n >= 2) & (den > 0)
            out[..., w, 0] = np.where(ok, (S * Std - St * Sd) / den, np.nan)
            out[..., w, 1] = np.where(ok, (Stt * Sd - St * Std) / den, np.nan)
            out[..., w, 2] = np.where(ok, np.sqrt(S / den), np.nan)
            ok0 = (n >= 1) & (Stt > 0)
            out[..., w, 3] = np.where(ok0, Std / Stt, np.nan)
            out[..., w, 4] = np.where(ok0, np.sqrt(np.float64(1) / Stt), np.nan)
            out[..., w, 5] = n
    return out


def fit_rows(win, par, wins, W, z, take_rows):
    """fit() with the rows left out (take_rows false) set to five NaN and n = -1."""
    out = fit(win, par, wins, W, z)
    out[~np.asarray(take_rows, bool)] = (np.nan,) * 5 + (-1.0,)
    return out


def reference(rows, ref, par, ranges, z, tab, mtr=None):
    """The whole contract from float32 rows [B][M][>= N] and ref [B][>= N], stage 2 from the checker's OWN plain FP64 stage 1
    (fp64_stage1): dict win [B][M][J][3], fit [B][M][W][6] (float64), undecided.  What the CPU tests and the seed search use."""
    wins = windows(par, ranges)
    B, M = rows.shape[:2]
    Fc, Fr = fp64_stage1(rows, par, wins, tab["g"]), fp64_stage1(ref, par, wins, tab["g"])
    s2 = stage2(Fc, Fr[:, None], par, tab)
    take, und = takes_part(s2, par)
    win = np.stack([s2[k].astype(np.float64) for k in ("delta", "err", "mcoh")], axis=-1)
    rows_in = np.ones((B, M), bool) if mtr is None else np.asarray(mtr) > 0
    win[~rows_in] = np.nan
    und_rows = s2["undecided"] + und if rows_in.all() else None
    if und_rows is None:  # only the rows that take part count
        s2 = stage2(Fc[rows_in], np.broadcast_to(Fr[:, None], Fc.shape)[rows_in], par, tab)
        und_rows = s2["undecided"] + takes_part(s2, par)[1]
    return dict(win=win, fit=fit_rows(win, par, wins, len(ranges), z, rows_in), undecided=und_rows, wins=wins)


def check(name, got, want, bound):
    """got (float64) inside want +- bound (longdouble), NaN exactly where want is NaN; prints and returns the largest |error| / bound."""
    got = np.asarray(got)
    nan = np.isnan(want.astype(np.float64))
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN positions differ ({int(np.isnan(got).sum())} against {int(nan.sum())})"
    err = np.abs(got[~nan].astype(LD) - want[~nan])
    b = bound[~nan]
    assert np.isfinite(b.astype(np.float64)).all(), f"{name}: an infinite bound"
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(err == 0, 0, err / b).astype(np.float64)
    worst = float(frac.max()) if frac.size else 0.0
    print(f"{name}: worst |error| / bound {worst:.3g} over {frac.size} values")
    assert worst <= 1, f"{name}: outside its bound ({worst:.3g})"
    return worst


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------------
# (i) L no multiple of 4, J = 73 no multiple of 16 or 32; (ii) the largest window and the widest table, Qx = 64; (iii) qa clips at 0, many items
SETS = {
    "i": (Par(100, 37, 128, 3, 20, h=2, taper=0.3, min_coh=0.5, max_err=5.0, max_delta=20.0, err_floor=1e-3),
          ((0, 1501), (700, 712), (661, 1501), (3, 611))),
    "ii": (Par(1024, 1024, 1024, 20, 68, h=8, taper=0.1, min_coh=0.2, err_floor=1e-4),
           ((0, 1501), (700, 712), (477, 1501), (3, 1100))),
    "iii": (Par(16, 1, 16, 1, 3, h=2, taper=1.0, min_coh=0.3, max_err=50.0, err_floor=1e-2),
            ((0, 1501), (700, 712), (1000, 1501), (3, 611))),
}


def parity_batch(seed, B=3, M=9):
    """wxs_rows_ref.parity_batch's construction: (rows float32 [B][M][N + 3], ref float32 [B][N + 1], counts uint32 [B][M]) with NaN pad
    columns; row m is the analytically stretched wavelet of its ensemble plus seeded noise of sigma 0, 0.2 or 1 (m % 3), scaled by
    1e-6 .. 1e2; row (0, 5) is all zero; the reference of ensemble 1 is zero inside [3, 611); the counts leave out 0 / 4 / 8 rows."""
    import wxs_rows_ref as wr
    return wr.parity_batch(seed, B, M)


# recovery: band-limited noise at N = 4096 and its copy at lag t (1 + REPS) by stretch_rows_ref's cubic convolution
RN, RZ, REPS = 4096, 2048.0, 1e-3
RTOL = 0.05   # of REPS, on eps_hat and eps0: the checker's own evaluation of this input is off by 3.3 % at the worst (test_mwcs_rows_cpu.py)
RPAR = Par(256, 64, 256, 16, 36, h=3, taper=0.2, min_coh=0.5, err_floor=1e-3)   # 0.0625 .. 0.14 cycles per sample
RRANGES = ((2148, 3048), (1048, 1948))   # 100 .. 1000 samples of lag on either side: |v delta| <= 2 pi 0.14 * 1e-3 * 1000 = 0.88 < pi


def recovery_rows(seed=0):
    """(ref float32 [RN], row float32 [RN]): white noise band-passed to 0.05 .. 0.15 cycles per sample; row(t) = ref(t (1 + REPS))."""
    import stretch_rows_ref as srr
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(RN))
    f = np.fft.rfftfreq(RN)
    X *= np.exp(-0.5 * ((f - 0.10) / 0.025) ** 2) * ((f > 0.05) & (f < 0.15))
    x = np.fft.irfft(X, RN)
    ref = (x / np.abs(x).max()).astype(np.float32)
    row = srr.stretched(ref, RZ, [REPS])[0][0].astype(np.float64).astype(np.float32)
    return ref, row
