"""The checker of tspws_hip_dtw_rows (include/tspws_hip.h: dv/v by dynamic time warping), in numpy float64.

dtw() implements the contract's definition literally: normalisation, error, accumulation, backtracking and fit, every operation a single
numpy float64 operation in the stated order (numpy contracts nothing), vectorised over rows and lags, with python loops over the samples i,
over k inside a slanted candidate, and over the backtrack.  Min-plus over individually rounded operations has one answer, so the device is
required to agree with it bit for bit: lags, dist and fit.  It also counts, per row, the samples at which the choice rule met a tie (the
smallest candidate attained by more than one of dc, dm, dp at some real lag).

brute() is independent of it: for tiny cases it enumerates every admissible lag sequence -- steps of 0 or +-1, every run between two changes
at least b samples long, the first and the last run at least 1 -- and sums e along each.

Also the inputs the tests share: the parameter sets, the lag ranges, the parity batch (wxs_rows_ref.parity_batch) and the recovery rows."""
import itertools

import numpy as np

N = 1501
Z = 750.0
ZS = (750.0, 0.0, 750.25)
INT_MIN = -2 ** 31
C_, MN, PL = 0, 1, 2

# name -> (Lmax, b): (i) one lag per lane, no ring; (ii) nl = 63 / 65, the lane-count edge (one lag per lane / two); (iii) four lags per lane
SETS = {"i": (5, 1), "ii63": (31, 3), "ii65": (32, 3), "iii": (127, 8)}
# touching both trace ends; of length 1; shorter than b = 3 and 8; overlapping the first, around the zeros of ensemble 1's reference [3, 611)
RANGES = ((0, N), (700, 701), (650, 652), (100, 700))


def errors(c, r, n0, n1, Lmax):
    """(e float64 [R][n][nl], dead bool [R]) of rows c float32 [R][>= N] against references r float32 [R][>= N] (steps 1 and 2)."""
    c, r = np.asarray(c, np.float32), np.asarray(r, np.float32)
    Nn = min(c.shape[1], r.shape[1])
    n = np.arange(n0, n1)
    k0, k1 = max(0, n0 - Lmax), min(Nn, n1 + Lmax)
    with np.errstate(all="ignore"):
        mc = np.abs(c[:, n0:n1]).max(axis=1)
        mr = np.abs(r[:, k0:k1]).max(axis=1)
        dead = ~(np.isfinite(mc) & np.isfinite(mr) & (mc > 0) & (mr > 0))      # (np.max propagates a NaN sample)
        ac, ar = np.float64(1.0) / mc.astype(np.float64), np.float64(1.0) / mr.astype(np.float64)
        idx = np.clip(n[:, None] + np.arange(-Lmax, Lmax + 1)[None, :], 0, Nn - 1)                  # [n][nl]
        cn = c[:, n0:n1].astype(np.float64) * ac[:, None]
        rn = r.astype(np.float64)[:, idx] * ar[:, None, None]
        d = cn[:, :, None] - rn
        e = d * d
    e[dead] = 0.0
    return e, dead


def accumulate(e, b):
    """(D_end [R][nl], choice uint8 [R][n][nl], ties int [R]) of e [R][n][nl] (step 3)."""
    R, n, nl = e.shape
    D = np.empty_like(e)
    ch = np.zeros(e.shape, np.uint8)
    ties = np.zeros(R, np.int64)
    inf = np.full((R, 1), np.inf)
    D[:, 0] = e[:, 0]
    for i in range(1, n):
        ib = max(0, i - b)
        V = D[:, ib].copy()
        for k in range(i - 1, ib, -1):
            V = V + e[:, k]
        dc = D[:, i - 1]
        dm = np.concatenate([inf, V[:, :-1]], axis=1)
        dp = np.concatenate([V[:, 1:], inf], axis=1)
        isc = (dc <= dm) & (dc <= dp)
        ism = ~isc & (dm <= dp)
        best = np.where(isc, dc, np.where(ism, dm, dp))
        ch[:, i] = np.where(isc, C_, np.where(ism, MN, PL))
        D[:, i] = e[:, i] + best
        ties += (((dc == best).astype(np.int8) + (dm == best) + (dp == best)) > 1).any(axis=1)
    return D[:, n - 1].copy(), ch, ties


def backtrack(D_end, ch, b, Lmax):
    """lag int32 [R][n] (step 4)."""
    R, n, nl = ch.shape
    lag = np.empty((R, n), np.int32)
    for r in range(R):
        li = int(np.argmin(D_end[r]))          # the first smallest
        i = n - 1
        lag[r, i] = li - Lmax
        c = ch[r]
        while i > 0:
            k = c[i, li]
            if k == C_:
                lag[r, i - 1] = li - Lmax
                i -= 1
            else:
                li += -1 if k == MN else 1
                ib = max(0, i - b)
                lag[r, ib:i] = li - Lmax
                i = ib
    return lag


def fit_of(lag, dist_num, n0, z, Lmax):
    """fit float64 [..][6] = eps_hat, icpt, err, rms, dist, clip of integer paths lag [..][n] with D[n-1][l*] = dist_num [..] (step 5)."""
    lag = np.asarray(lag).astype(np.int64)
    n = lag.shape[-1]
    i = np.arange(n, dtype=np.int64)
    f = np.float64
    S, Si, Sii = f(n), f(int(i.sum())), f(int((i * i).sum()))
    Sl, Sil, Sll = lag.sum(-1).astype(f), (i * lag).sum(-1).astype(f), (lag * lag).sum(-1).astype(f)
    clip = (np.abs(lag) == Lmax).sum(-1).astype(f)
    with np.errstate(all="ignore"):
        den = S * Sii - Si * Si
        num = S * Sil - Si * Sl
        eh = num / den
        t0 = (f(n0) - f(z)) + Si / S
        ic = Sl / S - eh * t0
        res = (Sll - (Sl / S) * Sl) - eh * (num / S)
        rms = np.sqrt(np.where(res > 0, res, 0.0) / S)
        err = rms * np.sqrt(S / den)
        dist = np.asarray(dist_num, f) / S
    return np.stack(np.broadcast_arrays(eh, ic, err, rms, dist, clip), axis=-1)


def dtw(c, r, n0, n1, Lmax, b, z):
    """The definition on rows c [R][>= N] against references r [R][>= N] for ONE range: dict(D_end [R][nl], choice [R][n][nl], lag int32
    [R][n], fit [R][6], dead [R], ties [R])."""
    e, dead = errors(c, r, n0, n1, Lmax)
    D_end, ch, ties = accumulate(e, b)
    lag = backtrack(D_end, ch, b, Lmax)
    fit = fit_of(lag, D_end[np.arange(len(lag)), lag[:, -1] + Lmax], n0, z, Lmax)
    fit[dead, :5] = np.nan
    fit[dead, 5] = -1
    lag[dead] = INT_MIN
    return dict(D_end=D_end, choice=ch, lag=lag, fit=fit, dead=dead, ties=ties, e=e)


def dtw_batch(rows, ref, mtr, ranges, Lmax, b, z):
    """(fit [B][M][W][6], lag int32 [B][M][T], ties [B][M][W], dead [B][M][W]) of a batch as Plan.dtw_rows takes it; rows left out by mtr
    give NaN, clip = -1 and INT_MIN."""
    B, M = rows.shape[:2]
    take = np.ones((B, M), bool) if mtr is None else np.asarray(mtr) > 0
    W = len(ranges)
    T = sum(n1 - n0 for n0, n1 in ranges)
    fit = np.full((B, M, W, 6), np.nan)
    fit[..., 5] = -1
    lag = np.full((B, M, T), INT_MIN, np.int32)
    ties = np.zeros((B, M, W), np.int64)
    dead = np.ones((B, M, W), bool)
    bi, mi = np.nonzero(take)
    off = 0
    for w, (n0, n1) in enumerate(ranges):
        o = dtw(rows[bi, mi], ref[bi], n0, n1, Lmax, b, z)
        fit[bi, mi, w] = o["fit"]
        lag[bi, mi, off:off + n1 - n0] = o["lag"]
        ties[bi, mi, w] = o["ties"]
        dead[bi, mi, w] = o["dead"]
        off += n1 - n0
    return fit, lag, ties, dead


def refit(lag, fit, ranges, Lmax, z):
    """The fit formula on given lags [..][T] with the dist of a given fit [..][W][6] (dist n_w recovers no numerator exactly, so dist is
    copied): what the device's own lags must give.  Paths of INT_MIN give NaN and clip = -1."""
    out = np.empty_like(fit)
    off = 0
    for w, (n0, n1) in enumerate(ranges):
        lg = lag[..., off:off + n1 - n0]
        deadw = (lg == INT_MIN).all(axis=-1)
        o = fit_of(np.where(lg == INT_MIN, 0, lg), np.zeros(lg.shape[:-1]), n0, z, Lmax)
        o[..., 4] = fit[..., w, 4]
        o[deadw, :5] = np.nan
        o[deadw, 5] = -1
        out[..., w, :] = o
        off += n1 - n0
    return out


def admissible(lag, b, Lmax):
    """Whether an integer path obeys the strain limit: steps of 0 or +-1 inside [-Lmax, Lmax]; every run between two changes at least b long."""
    lag = [int(v) for v in lag]
    if any(abs(v) > Lmax for v in lag) or any(abs(x - y) > 1 for x, y in zip(lag, lag[1:])):
        return False
    changes = [i for i in range(1, len(lag)) if lag[i] != lag[i - 1]]
    return all(y - x >= b for x, y in zip(changes, changes[1:]))


def brute(e, b):
    """(smallest cost, the set of paths attaining it as tuples of lag indices) over every admissible path, for e [n][nl]; tiny cases only."""
    n, nl = e.shape
    best, arg = None, set()
    for start in range(nl):
        for steps in itertools.product((0, -1, 1), repeat=n - 1):
            path = [start]
            for s in steps:
                path.append(path[-1] + s)
            if min(path) < 0 or max(path) >= nl:
                continue
            changes = [i for i in range(1, n) if steps[i - 1] != 0]
            if any(y - x < b for x, y in zip(changes, changes[1:])):
                continue
            cost = e[0, path[0]]
            for i in range(1, n):
                cost = cost + e[i, path[i]]
            if best is None or cost < best:
                best, arg = cost, {tuple(path)}
            elif cost == best:
                arg.add(tuple(path))
    return best, arg


def parity_batch(seed, B=3, M=9):
    """wxs_rows_ref.parity_batch's construction: (rows float32 [B][M][N + 3], ref float32 [B][N + 1], counts uint32 [B][M]) with NaN pad
    columns; scales of 1e-6 .. 1e2; row (0, 5) is all zero; the reference of ensemble 1 is zero inside [3, 611); the counts leave out
    0 / 4 / 8 rows."""
    import wxs_rows_ref as wr
    return wr.parity_batch(seed, B, M)


def well_posed(seed, B=3, M=9):
    """Whether the parity batch of `seed` exercises what the parity test names, judged by the checker alone under set (i): the all-zero row is
    dead in every range and no other participating row is; inside the range around the zeros of ensemble 1's reference the choice rule met
    ties on every participating row of ensemble 1; and no path of the long ranges is constant (the backtrack has slanted choices to follow)."""
    rows, ref, mtr = parity_batch(seed, B, M)
    Lmax, b = SETS["i"]
    fit, lag, ties, dead = dtw_batch(rows[:, :, :N], ref[:, :N], mtr, RANGES, Lmax, b, Z)
    take = mtr > 0
    want_dead = np.zeros((B, M), bool)
    want_dead[0, 5] = True
    ok = (dead[take] == want_dead[take][:, None]).all() and (ties[1][take[1]][:, 3] > 0).all()
    alive = take & ~want_dead
    return bool(ok and (lag[alive][:, :N].min(axis=1) < lag[alive][:, :N].max(axis=1)).all())


# recovery: a smooth reference at N = 1501 and cur(t) = ref(t (1 + eps)), eps = +-1e-2, z = 750, Lmax = 10, b = 4
REPS, RLMAX, RB = 1e-2, 10, 4
RRANGES = ((800, 1400), (100, 700))   # 50 .. 650 samples of lag on either side: |eps t| <= 6.5 < Lmax


def recovery_rows():
    """(ref float32 [N], rows float32 [2][N]): a sum of three slow sinusoids (periods of 37 to 91 samples: smooth against one sample of lag,
    with no repetition inside +-Lmax) and its copies at t (1 + REPS) and t (1 - REPS), evaluated analytically."""
    t = np.arange(N, dtype=np.float64) - Z

    def a(u):
        return np.sin(2 * np.pi * u / 37.0 + 0.3) + 0.7 * np.sin(2 * np.pi * u / 61.0 + 1.1) + 0.5 * np.sin(2 * np.pi * u / 91.0 + 2.0)
    return a(t).astype(np.float32), np.stack([a(t * (1 + REPS)), a(t * (1 - REPS))]).astype(np.float32)


def recovery_tolerance():
    """(tol [2][W], the checker's eps_hat [2][W]): the checker's own |eps_hat -+ REPS| on the recovery rows plus the integer-lag quantisation:
    a rounding error of variance 1/12 per sample in the n_w samples of a range moves the slope by 1 / sqrt(12 sum (i - mean)^2) =
    1 / sqrt(n_w (n_w^2 - 1)), at most 1 / (n_w sqrt(12)) times sqrt(12 / (n_w - 1/n_w)) -- the bound 1 / (n_w sqrt(12)) holds a fortiori."""
    ref, rows = recovery_rows()
    out = np.empty((2, len(RRANGES)))
    eh = np.empty((2, len(RRANGES)))
    for w, (n0, n1) in enumerate(RRANGES):
        o = dtw(rows, np.stack([ref, ref]), n0, n1, RLMAX, RB, Z)
        eh[:, w] = o["fit"][:, 0]
        out[:, w] = np.abs(eh[:, w] - np.array([REPS, -REPS])) + 1.0 / ((n1 - n0) * np.sqrt(12.0))
    return out, eh
