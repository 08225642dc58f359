"""The checker of the group-arrival calls (tspws_hip_ftan_coef / tspws_hip_ftan_rows): the contract's definition in numpy on coefficient sets.
It takes the frame and the window members from the wavelet cross-spectrum's checker (wxs_rows_ref.Frame, members).  No GPU import here.

Peaks and their five values are formed in float64 with the contract's operation order -- a2 = re re + im im, den = (am - 2 a0) + ap,
d = 0.5 (am - ap) / den, tg = (k + d) D - z, amp = sqrt(a0) -- every operation rounded on its own, as numpy rounds it: an implementation
that follows the contract gives the same bits, so the tests compare bit for bit.

The noise sum Q is formed in np.longdouble, and beside it a bound that a correct FP64 implementation stays inside WHATEVER the order of its
additions (wxs_rows_ref's rules): with u = 2**-53 a term a2 = re re + im im is two products and one addition, |a2 - a2*| <= b = 2.01 u a2*,
and n terms added in any order, each addition rounded, err by at most sum b + 1.01 (n - 1) u sum (a2* + b).  Participation must be decided
by the inputs: a term is left out iff a component is not finite; a term of finite components at or above 1e300 (where FP64 might overflow
and the exact value not) is counted in `undecided`, and the tests assert that there is none; then n is exact.  No tolerance is fitted to an
output."""
import numpy as np

from wxs_rows_ref import Frame, members  # noqa: F401  (the tests take them from here)

U = 2.0 ** -53
LD = np.longdouble
N, Z = 1501, 750.0
NAN = float("nan")


def a2_of(c):
    """a2 = re re + im im in float64, two products and one addition."""
    c = np.asarray(c, np.complex128)
    with np.errstate(over="ignore", invalid="ignore"):
        return c.real * c.real + c.imag * c.imag


def peaks_of(fr, s, ys, win, z, skip_wrapped, P):
    """[P][5] = tg, amp, re, im, k of the first P peaks of scale s (ys: its complex128 coefficients [Ns]) inside the window; unused slots
    hold four NaN and -1."""
    out = np.full((P, 5), NAN)
    out[:, 4] = -1.0
    Ns, D = int(fr.Ns[s]), np.float64(fr.D[s])
    a2 = a2_of(ys)
    k = members(fr, s, win, skip_wrapped)
    k = k[(k >= 1) & (k <= Ns - 2)]
    if not k.size:
        return out
    am, a0, ap = a2[k - 1], a2[k], a2[k + 1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(am) & np.isfinite(a0) & np.isfinite(ap) & (a0 > am) & (a0 >= ap)
    k, am, a0, ap = k[ok], am[ok], a0[ok], ap[ok]
    order = np.lexsort((k, -a0))[:P]          # decreasing a2, ties by increasing k
    k, am, a0, ap = k[order], am[order], a0[order], ap[order]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        den = (am - 2.0 * a0) + ap
        d = np.where(den != 0, 0.5 * (am - ap) / np.where(den != 0, den, 1.0), 0.0)
        tg = (k.astype(np.float64) + d) * D - np.float64(z)
        amp = np.sqrt(a0)
    n = k.size
    out[:n, 0], out[:n, 1], out[:n, 2], out[:n, 3], out[:n, 4] = tg, amp, ys[k].real, ys[k].imag, k
    return out


def noise_of(fr, s, ys, rng, skip_wrapped):
    """(Q* longdouble, bound longdouble, n, undecided) of scale s inside the noise range."""
    k = members(fr, s, rng, skip_wrapped)
    c = ys[k]
    fin = np.isfinite(c.real) & np.isfinite(c.imag)
    re, im = c.real[fin].astype(LD), c.imag[fin].astype(LD)
    t = re * re + im * im
    undecided = int((t >= LD(1e300)).sum())
    b = LD(2.01) * LD(U) * t
    n = int(fin.sum())
    return t.sum(), b.sum() + LD(1.01) * max(n - 1, 0) * LD(U) * (t + b).sum(), n, undecided


def reference(fr, Y, z, windows, scales, P, ens=None, skip_wrapped=False, noise=None, take=None):
    """dict for the sets Y [nrow][ncoef] (complex128): peaks float64 [nrow][W][Sx][P][5]; with `noise` Q and b_Q (longdouble [nrow][Sx]; NaN
    for the rows with take[i] false), n (float64 [nrow][Sx]; -1 there) and undecided.  windows is [B][W][2] (or [W][2] for all), noise
    [B][2] (or a pair); ens[i] names the ensemble of row i (None: row i is ensemble i)."""
    nrow = Y.shape[0]
    s0, s1 = scales
    windows = np.asarray(windows)
    Wn = windows.shape[-2]
    peaks = np.full((nrow, Wn, s1 - s0, P, 5), NAN)
    peaks[..., 4] = -1.0
    Q, bQ, n = np.full((nrow, s1 - s0), LD("nan")), np.full((nrow, s1 - s0), LD("nan")), np.full((nrow, s1 - s0), -1.0)
    undecided = 0
    for i in range(nrow):
        if take is not None and not take[i]:
            continue
        b = i if ens is None else int(ens[i])
        wins = windows if windows.ndim == 2 else windows[b]
        for s in range(s0, s1):
            ys = Y[i, fr.off[s]:fr.off[s + 1]]
            for w in range(Wn):
                peaks[i, w, s - s0] = peaks_of(fr, s, ys, wins[w], z, skip_wrapped, P)
            if noise is not None:
                rng = np.asarray(noise)
                Q[i, s - s0], bQ[i, s - s0], n[i, s - s0], und = noise_of(fr, s, ys, rng if rng.ndim == 1 else rng[b], skip_wrapped)
                undecided += und
    return dict(peaks=peaks, Q=Q, b_Q=bQ, n=n, undecided=undecided)


def same(a, b):
    """Bit equality of two float64 arrays, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def check_noise(got, want, what=""):
    """got float64 [..][Sx][2] against the checker: n exact, NaN exactly where the checker has NaN, Q inside its bound.  Prints the largest
    |error| / bound before it asserts and returns it."""
    got = np.asarray(got, np.float64)
    Q, b, n = (want[k].reshape(got.shape[:-1]) for k in ("Q", "b_Q", "n"))
    assert want["undecided"] == 0, f"{what}: {want['undecided']} terms whose participation the inputs do not decide"
    dead = n < 0
    assert np.array_equal(np.isnan(got[..., 0]), dead), f"{what}: NaN positions of Q differ"
    assert np.array_equal(got[..., 1], n), f"{what}: n differs"
    err = np.abs(got[..., 0][~dead].astype(LD) - Q[~dead])
    bb = b[~dead]
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(err == 0, 0, err / bb).astype(np.float64)  # (an error against a zero bound: inf)
    worst = float(frac.max()) if frac.size else 0.0
    print(what, f"Q: worst |error| / bound {worst:.3g} over {frac.size} sums")
    assert worst <= 1, f"{what}: a noise sum outside its bound ({worst})"
    return worst


def expected_stats(fr, windows, noise, scales, skip, B, rows, left_out, rounds=1):
    """The stats from the definition: the classes of ensembles with equal tables, and per class the members of every (scale, window) and
    (scale, noise range) in segments of 256."""
    windows = np.asarray(windows)
    windows = np.broadcast_to(windows, (B,) + windows.shape[-2:])
    nz = None if noise is None else np.broadcast_to(np.asarray(noise), (B, 2))
    keys = []
    for b in range(B):
        key = (windows[b].tobytes(), None if nz is None else nz[b].tobytes())
        if key not in keys:
            keys.append(key)
    items = 0
    for wb, nb in keys:
        rngs = [tuple(r) for r in np.frombuffer(wb, windows.dtype).reshape(-1, 2)] + ([] if nb is None else [tuple(np.frombuffer(nb, nz.dtype))])
        items += sum(-(-members(fr, s, r, skip).size // 256) for s in range(*scales) for r in rngs)
    return dict(rounds=rounds, rows=rows, left_out=left_out, items=items, classes=len(keys))


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------------
# per ensemble W = 2 windows whose edges are no multiples of any D; ensembles 0 and 2 share their tables (one class), ensemble 1 has others
PWIN = np.array([[[803, 1307], [191, 701]], [[777, 1203], [5, 1499]], [[803, 1307], [191, 701]]], np.int64)
PNOISE = np.array([[1311, 1501], [1207, 1493], [1311, 1501]], np.int64)
ZS = (750.0, 750.25)
B, M = 3, 5


def parity_batch(seed, B=B, M=M):
    """(rows float32 [B][M][N + 3] with NaN pad columns, counts uint32 [B][M]): ensemble b is a sum of three Gaussian wave packets of
    different carriers arriving at different lags on both sides of z; row m adds seeded noise of sigma 0.05, 0.3 or 1 (m % 3) and a scale of
    1e-3 .. 1e2.  The counts leave out 0 / 2 / 4 rows."""
    rng = np.random.default_rng(seed)
    rows = np.full((B, M, N + 3), np.nan, np.float32)
    t = np.arange(N, dtype=np.float64) - Z
    for b in range(B):
        sig = np.zeros(N)
        for f, lag, sg in ((0.21, 180.0, 14.0), (0.09, 260.0, 30.0), (0.035, 390.0, 70.0)):
            lag = lag * (1 + 0.1 * b)
            for side in (1.0, -0.8):
                sig += abs(side) * np.exp(-0.5 * ((t - np.sign(side) * lag) / sg) ** 2) * np.cos(2 * np.pi * f * (t - np.sign(side) * lag) + 0.3 * b)
        for m in range(M):
            x = sig + (0.05, 0.3, 1.0)[m % 3] * rng.standard_normal(N)
            rows[b, m, :N] = x * 10.0 ** rng.uniform(-3, 2)
    mtr = np.full((B, M), 7, np.uint32)
    if B > 2:
        mtr[1, 1:4:2] = 0   # 2 rows left out
        mtr[2] = 0
        mtr[2, 3] = 2       # one row takes part
    return rows, mtr


# constructed sets: everything zero but chosen coefficients of scale CS; window CWIN[0] has the members CK0 .. CK0 + 511 of that scale (two
# whole segments), CWIN[1] is the whole trace
CS, CK0 = 0, 100
CNAMES = ("equal", "plateau", "borders_a", "borders_b", "ends", "many", "inf_nan", "den0", "zero")


def constructed(fr):
    """(Y complex128 [9][ncoef], windows [2][2], noise pair, want: dict name -> the k of ALL peaks of (window 0, scale CS) in order; CWHOLE: where the whole-trace window's differ).  The
    rows, by CNAMES: two peaks of equal a2 and a smaller third; a plateau; peaks at members 0, 255 and 511 of window 0 (its first and last
    member, a segment's last); at members 256 (a segment's first) and 510; large values at k = 0 and Ns - 1 with one true peak (fewer than
    P); seven peaks over both segments (more than P); an Inf and a NaN coefficient beside would-be peaks, and one true peak; a peak with
    den == 0; all zero."""
    D, Ns = int(fr.D[CS]), int(fr.Ns[CS])
    assert D == 2 and Ns == 751 and fr.N == N
    win = np.array([[CK0 * D - 1, (CK0 + 512) * D - 1], [0, N]], np.int64)
    assert np.array_equal(members(fr, CS, win[0], False), np.arange(CK0, CK0 + 512))
    Y = np.zeros((len(CNAMES), fr.ncoef), np.complex128)
    o = int(fr.off[CS])
    row = {n: Y[i, o:o + Ns] for i, n in enumerate(CNAMES)}
    row["equal"][[150, 300, 400]] = (3 + 4j, 5 + 0j, 4 - 2j)
    row["plateau"][[200, 201]] = (2 + 0j, 0 - 2j)
    row["borders_a"][[CK0, CK0 + 255, CK0 + 511]] = (1 + 1j, 2 + 1j, 3 + 1j)
    row["borders_b"][[CK0 + 256, CK0 + 510, CK0 + 511]] = (1 - 1j, 2 - 1j, 0.5 + 0j)
    row["ends"][[0, 1, 5, Ns - 2, Ns - 1]] = (9 + 0j, 1 + 0j, 0.25 + 0.5j, 1 + 0j, 9 + 0j)
    for j, k in enumerate((110, 120, 131, 300, 355, 357, 600)):
        row["many"][k] = (1 + j % 4) + 0.5j * (j + 1)
    row["inf_nan"][[249, 250, 251, 399, 400, 401, 500]] = (3, complex(np.inf, 0), 2, 3, complex(0, np.nan), 2, 1 + 1j)
    row["den0"][[320, 321, 322]] = (complex(1, 1 - 2.0 ** -53), 1 + 1j, 1 + 1j)
    want = dict(equal=[150, 300, 400], plateau=[200], borders_a=[CK0 + 511, CK0 + 255, CK0], borders_b=[CK0 + 510, CK0 + 256], ends=[],
                many=[600, 300, 357, 131, 355, 120, 110], inf_nan=[500], den0=[321], zero=[])
    return Y, win, np.array([3, 1201], np.int64), want


CWHOLE = dict(ends=[5])  # the peaks inside the whole-trace window where they differ from window 0's


# recovery: Gaussian wave packets at the scales 4, 8, .., 24 of the default frame at N = 4096
RN, RZ = 4096, 2048.0
RSCALES = tuple(range(4, 25, 4))
RWIN = np.array([[2148, 4096]], np.int64)


def recovery_row(fr):
    """(row float32 [RN], t0 per scale of RSCALES): the sum over those scales of exp(-0.5 ((t - t0) / sg)^2) cos(omega_s (t - t0) + 0.7)
    with sg = 1.5 scale_s and t0 = z + 300.3 + 40 s."""
    t = np.arange(RN, dtype=np.float64)
    x = np.zeros(RN)
    t0s = []
    for s in RSCALES:
        t0, sg = RZ + 300.3 + 40 * s, 1.5 * fr.scale[s]
        x += np.exp(-0.5 * ((t - t0) / sg) ** 2) * np.cos(fr.omega[s] * (t - t0) + 0.7)
        t0s.append(t0)
    return x.astype(np.float32), np.array(t0s)


def check_recovery(fr, peaks, t0s, what=""):
    """peaks [1][Sx = S][1][5] of the recovery row (all scales, P = 1): |tg + z - t0| <= 0.25 D_s at every scale of RSCALES.  Prints the
    values and returns the worst error in units of D_s."""
    worst = 0.0
    for s, t0 in zip(RSCALES, t0s):
        tg, amp, k = peaks[0, s, 0, 0], peaks[0, s, 0, 1], peaks[0, s, 0, 4]
        e = abs(tg + RZ - t0) / fr.D[s]
        # (printed, not asserted: the phase of the coefficient at the peak against omega_s (k D_s - t0) + 0.7 of the packet)
        dphi = (np.arctan2(peaks[0, s, 0, 3], peaks[0, s, 0, 2]) - (fr.omega[s] * (k * fr.D[s] - t0) + 0.7) + np.pi) % (2 * np.pi) - np.pi
        print(f"{what} s = {s}: D = {fr.D[s]}, t0 = {t0:.1f}, k = {k:.0f}, tg + z = {tg + RZ:.3f}, amp = {amp:.4g}, |error| = {e:.3f} D_s, phase off by {dphi:+.4f} rad")
        worst = max(worst, e)
    assert worst <= 0.25, f"{what}: a group arrival off by {worst} D_s"
    return worst
