"""The checker of the stretching call (tspws_hip_stretch_rows): from the float32 inputs it computes u, i and f in FP64 exactly as the
contract states them (three operations, each rounded; f = u - floor(u) is exact), and everything after that in np.longdouble: the weights,
the stretched reference S*, the three window sums and cc*.  Beside every cc* it gives a bound that a correct FP64 implementation stays
inside WHATEVER the order of its operations.  With u = 2**-53, n the window length, r_k the four reference samples, c the row:

  weights   every w_k is a cubic in f in [0, 1) evaluated with at most 5 rounded operations whose intermediate values stay within 2.5 in
            magnitude (|1.5 f - 2.5| <= 2.5 is the largest), and an earlier error is multiplied by at most 2.5 afterwards only when f f is
            formed first (one rounding, error u); otherwise by f <= 1.  So |w_k - w_k*| <= 5 * 2.5 u (1 + small) < 13 u, absolute: the
            weights that vanish at f -> 1 or f -> 0 have no relative bound, and need none.
  S         four products and three additions on top: |S - S*| <= b_S = 1.01 u (13 sum |r_k| + 4 sum |w_k* r_k|)
  dot       |dot - dot*| <= b_dot = sum |c| b_S + 1.01 n u sum |c| (|S*| + b_S)    the error of S, then n roundings per term of the sum
            (one product, fused or not, and at most n - 1 additions; pad columns add exact zeros)
  sum S^2   |q - q*| <= b_q = sum (2 |S*| b_S + b_S^2) + 1.01 n u sum (|S*| + b_S)^2
  sum c^2   |x - x*| <= b_x = 1.01 n u x*                                           squares of floats are exact in FP64
  cc        cc = dot / sqrt(x) / sqrt(q) with two roots and two divisions, 4 more roundings.  With r_x = b_x / x*, r_q = b_q / q* < 1:
            |cc - cc*| <= b_cc = ((|dot*| + b_dot) (1 - r_x)^-1/2 (1 - r_q)^-1/2 (1 + 4.04 u) - |dot*|) / sqrt(x* q*)
            -- no first-order step; r_x >= 1 or r_q >= 1 gives an infinite bound (the tests assert that theirs are finite).

No tolerance is fitted to an output.  A dead row (x* == 0) or a dead stretched reference (q* == 0) has cc* = NaN, and so has every entry of
a row that does not take part; the NaN positions must agree.  (The longdouble evaluation itself errs by about 2**-64 n: four thousand times
below the bounds.)"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
N, Z = 1501, 750.0
WINDOWS = ((3, 611), (890, 1501), (0, 1501))
EPS0 = (0.0037, -0.00612, 0.0)


# ---- the analytic rows of the tests --------------------------------------------------------------------------------------------------
def wavelet(seed):
    """a(t) = sum_{k<6} A_k sin(2 pi f_k t + phi_k) exp(-|t| / 400), seeded A in [0.5, 1], f in [0.03, 0.08] cycles per sample."""
    rng = np.random.default_rng(seed)
    A, f, ph = rng.uniform(0.5, 1, 6), rng.uniform(0.03, 0.08, 6), rng.uniform(0, 2 * np.pi, 6)

    def a(t):
        t = np.asarray(t, dtype=np.float64)
        return (A[:, None] * np.sin(2 * np.pi * f[:, None] * t[None, :] + ph[:, None])).sum(axis=0) * np.exp(-np.abs(t) / 400)
    return a


def analytic_rows(seed, n=N, z=Z, eps0=EPS0):
    """(ref float32 [n], rows float32 [len(eps0)][n]): ref = a(n - z), row j = a((n - z)(1 + eps0[j])), evaluated analytically."""
    a = wavelet(seed)
    t = np.arange(n, dtype=np.float64) - z
    return a(t).astype(np.float32), np.stack([a(t * (1 + e)) for e in eps0]).astype(np.float32)


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def positions(n, z, eps):
    """(i int64 [E][n], f float64 [E][n]) of the contract: u = n + (n - z) eps in FP64, every operation rounded on its own."""
    nn = np.arange(n, dtype=np.float64)[None, :]
    e = np.asarray(eps, dtype=np.float64)[:, None]
    u = nn + (nn - np.float64(z)) * e
    fl = np.floor(u)
    inside = (u >= -2.0) & (u < n + 1.0)  # (outside: all four samples lie outside [0, n); z may be huge)
    return np.where(inside, fl, -4).astype(np.int64), np.where(inside, u - fl, 0.0)


def weights(f):
    """The four cubic-convolution weights (Keys, a = -1/2) in the type of f, as the contract writes them."""
    return (((-0.5 * f + 1) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1, ((-1.5 * f + 2) * f + 0.5) * f, (0.5 * f - 0.5) * f * f)


def taps(ref, i, dtype):
    """ref[i - 1 .. i + 2] as four [E][n] arrays of `dtype`, zero outside [0, n)."""
    n = ref.shape[0]
    r = np.concatenate([ref.astype(dtype), np.zeros(1, dtype)])  # (index n: the zero sample)
    out = []
    for k in (-1, 0, 1, 2):
        j = i + k
        out.append(r[np.where((j >= 0) & (j < n), j, n)])
    return out


def stretched(ref, z, eps):
    """(S* longdouble [E][n], b_S longdouble [E][n]) of one float32 reference row."""
    i, f = positions(ref.shape[0], z, eps)
    w = weights(f.astype(LD))
    r = taps(ref, i, LD)
    S = ((w[0] * r[0] + w[1] * r[1]) + w[2] * r[2]) + w[3] * r[3]
    bS = LD(1.01) * LD(U) * (13 * sum(np.abs(x) for x in r) + 4 * sum(np.abs(a * x) for a, x in zip(w, r)))
    return S, bS


def reference(rows, ref, z, eps, windows, mtr=None):
    """dict of [B][M][W][E] arrays for float32 rows [B][M][>= n] and ref [B][>= n], n = the plan's trace length = ref.shape[-1]: cc
    (longdouble, NaN for dead rows, dead stretched references and rows left out), b_cc (longdouble), and argmax [B][M][W] (the first index
    of the largest cc*, -1 without one)."""
    B, M = rows.shape[:2]
    n = ref.shape[-1]
    W, E = len(windows), len(eps)
    cc = np.full((B, M, W, E), np.nan, LD)
    bcc = np.full((B, M, W, E), np.nan, LD)
    for b in range(B):
        S, bS = stretched(ref[b, :n], z, eps)
        for w, (n0, n1) in enumerate(windows):
            nw = n1 - n0
            Sw, bw = S[:, n0:n1], bS[:, n0:n1]
            aS = np.abs(Sw) + bw
            q = (Sw * Sw).sum(axis=1)
            bq = (2 * np.abs(Sw) * bw + bw * bw).sum(axis=1) + LD(1.01) * nw * LD(U) * (aS * aS).sum(axis=1)
            for m in range(M):
                if mtr is not None and not mtr[b, m] > 0:
                    continue
                c = rows[b, m, n0:n1].astype(LD)
                ac = np.abs(c)
                x = (c * c).sum()
                dot = (Sw * c[None, :]).sum(axis=1)
                bdot = (bw * ac[None, :]).sum(axis=1) + LD(1.01) * nw * LD(U) * (aS * ac[None, :]).sum(axis=1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    cc[b, m, w] = dot / np.sqrt(x) / np.sqrt(q)
                    rx, rq = LD(1.01) * nw * LD(U), bq / q
                    ok = rq < 1
                    grow = 1 / np.sqrt((1 - rx) * np.where(ok, 1 - rq, 1)) * (1 + LD(4.04) * LD(U))
                    bound = ((np.abs(dot) + bdot) * grow - np.abs(dot)) / np.sqrt(x * q)
                bcc[b, m, w] = np.where(ok, bound, np.inf)
    live = ~np.isnan(cc.astype(np.float64))
    arg = np.where(live.any(axis=-1), np.argmax(np.where(live, cc, -np.inf), axis=-1), -1)
    return dict(cc=cc, b_cc=bcc, argmax=arg)


def margins_ok(want):
    """No (row, window) whose two largest cc* are closer than the sum of their bounds: the argmax is then decided by the inputs."""
    cc, b = want["cc"], want["b_cc"]
    live = ~np.isnan(cc.astype(np.float64))
    lo = np.where(live, cc - b, -np.inf)
    top = np.take_along_axis(lo, np.maximum(want["argmax"], 0)[..., None], axis=-1)  # the winner's lower end
    hi = np.where(live, cc + b, -np.inf)
    np.put_along_axis(hi, np.maximum(want["argmax"], 0)[..., None], -np.inf, axis=-1)
    return bool((hi.max(axis=-1, keepdims=True) < top)[want["argmax"][..., None] >= 0].all())


def check(cc, want, what=""):
    """Every entry of float64 `cc` [B][M][W][E] inside its bound around cc*, NaN exactly where cc* is NaN.  Prints the worst figure as a
    fraction of its bound before it asserts."""
    cc = np.asarray(cc)
    assert cc.shape == want["cc"].shape, (cc.shape, want["cc"].shape)
    nan = np.isnan(want["cc"].astype(np.float64))
    assert np.array_equal(np.isnan(cc), nan), f"{what}: NaN positions of cc differ"
    assert np.isfinite(want["b_cc"][~nan].astype(np.float64)).all(), f"{what}: an infinite bound"
    err = np.abs(cc[~nan].astype(LD) - want["cc"][~nan])
    frac = np.where(err == 0, 0, err / want["b_cc"][~nan])
    worst = float(frac.max()) if frac.size else 0.0
    print(what, f"worst |cc - cc*| / bound: {worst:.3g}; largest |cc - cc*| {float(err.max()) if err.size else 0:.3g}; "
          f"largest bound {float(want['b_cc'][~nan].max()) if err.size else 0:.3g}")
    assert worst <= 1, f"{what}: cc outside its bound ({worst:.3g} of it)"


def fit(cc, eps):
    """The contract's fit in numpy float64 on a float64 cc plane [..][E]: [..][4] = eps_hat, cc_hat, e*, edge."""
    cc = np.asarray(cc, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    E = eps.size
    out = np.empty(cc.shape[:-1] + (4,), np.float64)
    for idx in np.ndindex(*cc.shape[:-1]):
        c = cc[idx]
        live = ~np.isnan(c)
        if not live.any():
            out[idx] = (np.nan, np.nan, -1.0, 1.0)
            continue
        e = int(np.argmax(np.where(live, c, -np.inf)))
        res = (eps[e], c[e], float(e), 1.0)
        if 0 < e < E - 1:
            cm, c0, cp = c[e - 1], c[e], c[e + 1]
            with np.errstate(invalid="ignore"):
                den = cm - np.float64(2.0) * c0 + cp
                if den != 0:
                    d = np.float64(0.5) * (cm - cp) / den
                    step = eps[e + 1] - eps[e] if d >= 0 else eps[e] - eps[e - 1]
                    res = (eps[e] + d * step, c0 - np.float64(0.25) * (cm - cp) * d, float(e), 0.0)
        out[idx] = res
    return out


# ---- a plain FP64 evaluation in several orders (the checker's own test) -----------------------------------------------------------------
def _sum(v, order):
    """Sum of float64 [..][n] along the last axis in FP64: 'forward' / 'reversed' one by one, 'pairwise' by halves."""
    if order == "pairwise":
        while v.shape[-1] > 1:
            if v.shape[-1] % 2:
                v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], axis=-1)
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0]
    if order == "reversed":
        v = v[..., ::-1]
    return np.cumsum(v, axis=-1)[..., -1]  # (cumsum adds one by one, in order)


def fp64_cc(rows, ref, z, eps, windows, order="forward"):
    """cc float64 [M][W][E] of float32 rows [M][n] against one float32 ref [n], every operation in FP64, the sums in `order`."""
    i, f = positions(ref.shape[0], z, eps)
    w = weights(f)
    r = taps(ref, i, np.float64)
    S = ((w[0] * r[0] + w[1] * r[1]) + w[2] * r[2]) + w[3] * r[3]
    out = np.empty((rows.shape[0], len(windows), len(eps)))
    for k, (n0, n1) in enumerate(windows):
        c = rows[:, n0:n1].astype(np.float64)
        Sw = S[:, n0:n1]
        dot = _sum(c[:, None, :] * Sw[None, :, :], order)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, k, :] = dot / np.sqrt(_sum(c * c, order))[:, None] / np.sqrt(_sum(Sw * Sw, order))[None, :]
    return out
