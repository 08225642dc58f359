"""CPU reference for the inverse frame transform, scale by scale, with a bound at every output sample, and the checker that holds device rows
to it (tests/test_inverse_rows_gpu.py; the checker itself is tested in tests/test_inverse_rows_cpu.py).  No GPU import here.

For scale s of a frame (tables D, L, cd, N_s, scale; dual taps wd; gain_s = ln 2 / (2 Cpsi V scale_s)) and its coefficients y_s[0 .. N_s):

    x_s[n] = gain_s D_s sum_{k < N_s, 0 <= l < L_s, (k D_s + cd_s - l) mod N == n} Re(conj(wd_s[l]) y_s[k])
    B_s[n] = the same scatter of |Re wd||Re y| + |Im wd||Im y|

both formed in np.longdouble (reference wavelet_v7.c:138-147, cdotx.c:305-340 / :176-211: a tap runs from the zero-stuffed position k D of
its coefficient and wraps at the circular seam, where the grid restarts).  The taps are the ones handed in -- the device's own
(Plan.taps()) on the GPU, the oracle's on the CPU -- so tap generation stays out of the bound (test_frame_matches_oracle holds it to 1e-14).

The bounds use no number of their own:

    b_s[n] = (2 T_s + 6) 2^-52 B_s[n],    T_s = ceil(L_s / D_s) + 1

is the first-order bound of a dot product of 2 T_s multiply-adds in any order, with 6 more roundings for the gain, its product with D, the
scaled tap and the conversions, at 2^-52 instead of the unit roundoff 2^-53 to pay for second order.  A row that is a sum over all S scales
is held to sum_s b_s[n] + S 2^-52 sum_s |x_s[n]| (the second term: the combining kernel's additions).  An impulse set has ONE coefficient
with ONE non-zero component, so every output is at most one product: 4 * 2^-52 * |term|.

A bound that is too loose would hide a failure, so reference_rows asserts max_n b_s[n] / max_n |x_s[n]| < 1e-12 (CAP: a tenth of the suite's
TOL64 = 1e-11) for every scale of every set: every sample is held at least ten times tighter, per scale, than the one global
relerr(x, x_oracle) < 1e-11 on the sum over scales that the suite had before."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

CAP = 1e-12
TOL64 = 1e-11
LD = np.longdouble
EPS = LD(2.0) ** -52
INV_R = 8             # outputs per lane of k_inv_poly (csrc/inv_poly.h)


def _workers():
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


class Frame:
    """What the reference needs of a frame: N, the resolved V, Cpsi, the tables (dict of scale, L, cd, D, Ns) and the dual taps wd."""

    def __init__(self, N, V, Cpsi, tables, wd):
        self.N, self.V, self.Cpsi = int(N), int(V), float(Cpsi)
        self.scale = np.asarray(tables["scale"], np.float64)
        self.D, self.L, self.Ns, self.cd = (np.asarray(tables[k]).astype(np.int64) for k in ("D", "L", "Ns", "cd"))
        self.S = len(self.D)
        self.off = np.concatenate([[0], np.cumsum(self.Ns)]).astype(np.int64)
        self.toff = np.concatenate([[0], np.cumsum(self.L)]).astype(np.int64)
        self.ncoef = int(self.off[-1])
        self.wd = np.asarray(wd, np.complex128)
        assert self.wd.size == self.toff[-1]
        self.gain = LD(np.log(LD(2))) / (LD(2) * LD(self.Cpsi) * LD(self.V) * self.scale.astype(LD))
        self.T = -(-self.L // self.D) + 1

    @classmethod
    def from_oracle(cls, p, N):
        """The oracle's frame of the RESOLVED parameter set p (its tables are the device's: test_frame_matches_oracle)."""
        import abi
        f = abi.OracleFrame.from_params(p, N)
        t = dict(scale=f.scale, L=f.L, cd=f.cd, D=f.D, Ns=f.Ns)
        fr = cls(N, p.V, f.Cpsi, t, f.taps()[1])
        fr.oracle = f
        return fr

    @classmethod
    def from_plan(cls, pl):
        return cls(pl.N, pl.info.V, pl.Cpsi, pl.tables(), pl.taps()[1])


def scale_rows(fr, s, y, wd=None):
    """(x_s, B_s) as longdouble [nset][N] for the coefficients y[nset][N_s] of scale s (wd: other dual taps for this scale)."""
    N, D, L, Ns, cd = fr.N, int(fr.D[s]), int(fr.L[s]), int(fr.Ns[s]), int(fr.cd[s])
    w = fr.wd[fr.toff[s]: fr.toff[s + 1]] if wd is None else wd
    y = np.atleast_2d(y)
    assert y.shape[1] == Ns and w.size == L
    wr, wi = w.real.astype(LD), w.imag.astype(LD)
    yr, yi = y.real.astype(LD), y.imag.astype(LD)
    awr, awi, ayr, ayi = np.abs(wr), np.abs(wi), np.abs(yr), np.abs(yi)
    x, B = np.zeros((y.shape[0], N), LD), np.zeros((y.shape[0], N), LD)
    if L <= Ns:          # one tap at a time: the N_s outputs (k D + cd - l) mod N of a tap are distinct ((N_s - 1) D < N)
        base = np.arange(Ns, dtype=np.int64) * D + cd
        for l in range(L):
            n = (base - l) % N
            x[:, n] += wr[l] * yr + wi[l] * yi
            B[:, n] += awr[l] * ayr + awi[l] * ayi
    else:                # one coefficient at a time: its L <= N outputs are distinct
        lv = np.arange(L, dtype=np.int64)
        for k in range(Ns):
            n = (k * D + cd - lv) % N
            x[:, n] += wr[None, :] * yr[:, k, None] + wi[None, :] * yi[:, k, None]
            B[:, n] += awr[None, :] * ayr[:, k, None] + awi[None, :] * ayi[:, k, None]
    g = fr.gain[s] * LD(D)
    return g * x, g * B


def impulse_row(fr, s, k, value):
    """(x, bound) of the set whose only coefficient is `value` (one non-zero component) at index k of scale s."""
    assert (value.real == 0) != (value.imag == 0)
    N, D, L, cd = fr.N, int(fr.D[s]), int(fr.L[s]), int(fr.cd[s])
    w = fr.wd[fr.toff[s]: fr.toff[s + 1]]
    term = fr.gain[s] * LD(D) * (w.real.astype(LD) * LD(value.real) + w.imag.astype(LD) * LD(value.imag))
    x = np.zeros(N, LD)
    x[(k * D + cd - np.arange(L, dtype=np.int64)) % N] = term
    return x, 4 * EPS * np.abs(x)


class RowsRef:
    """want[R][N] (longdouble), bound[R][N] (longdouble), kinds[R] = ("full",) / ("scale", s) / ("impulse", s, k) / ("zero",), the frame and
    the cap ratio max_s max_n b_s / max_n |x_s| over the sets with data."""

    def __init__(self, fr, want, bound, kinds, cap_ratio):
        self.fr, self.want, self.bound, self.kinds, self.cap_ratio = fr, want, bound, kinds, cap_ratio
        self.R, self.N = want.shape


def reference_rows(fr, sets):
    """Reference rows and bounds of a list of coefficient sets: ("full", Y[ncoef]), ("scale", s, y[N_s]) -- scale s alone --,
    ("impulse", s, k, value) and ("zero",).  Consecutive full sets share the work per scale; so do the single-scale sets of one scale."""
    R, N, S = len(sets), fr.N, fr.S
    want, bound = np.zeros((R, N), LD), np.zeros((R, N), LD)
    sum_abs = np.zeros((R, N), LD)
    full = [r for r, st in enumerate(sets) if st[0] == "full"]
    single = {}
    for r, st in enumerate(sets):
        if st[0] == "scale":
            single.setdefault(st[1], []).append(r)
    cap = [0.0]

    def one_scale(s):
        rows = full + single.get(s, [])
        if not rows:
            return s, rows, None, None
        y = np.stack([sets[r][1][fr.off[s]: fr.off[s + 1]] if sets[r][0] == "full" else sets[r][2] for r in rows])
        x, B = scale_rows(fr, s, y)
        return s, rows, x, (2 * int(fr.T[s]) + 6) * EPS * B

    with ThreadPoolExecutor(_workers()) as pool:        # (numpy releases the GIL inside the long array operations)
        for s, rows, x, b in pool.map(one_scale, range(S)):
            if not rows:
                continue
            mx = np.abs(x).max(axis=1)
            assert (mx > 0).all(), f"scale {s}: a set without data in this scale has no cap ratio -- give it other data"
            ratio = float((b.max(axis=1) / mx).max())
            assert ratio < CAP, (f"scale {s} (D = {int(fr.D[s])}, L = {int(fr.L[s])}, N_s = {int(fr.Ns[s])}): max b_s / max |x_s| = {ratio:.3g} is not "
                                 f"below {CAP:g}: give the case other data or a smaller J, not a wider cap")
            cap[0] = max(cap[0], ratio)
            for i, r in enumerate(rows):
                want[r] += x[i]
                bound[r] += b[i]
                sum_abs[r] += np.abs(x[i])
    for r in full:
        bound[r] += S * EPS * sum_abs[r]
    for r, st in enumerate(sets):
        if st[0] == "impulse":
            want[r], bound[r] = impulse_row(fr, st[1], st[2], st[3])
    kinds = [tuple(st[:1]) if st[0] in ("full", "zero") else (st[0], st[1]) if st[0] == "scale" else (st[0], st[1], st[2]) for st in sets]
    return RowsRef(fr, want, bound, kinds, cap[0])


def assemble(fr, sets):
    """The coefficient sets as one complex128 array [R][ncoef] (what tspws_hip_inverse reads)."""
    Y = np.zeros((len(sets), fr.ncoef), np.complex128)
    for r, st in enumerate(sets):
        if st[0] == "full":
            Y[r] = st[1]
        elif st[0] == "scale":
            Y[r, fr.off[st[1]]: fr.off[st[1] + 1]] = st[2]
        elif st[0] == "impulse":
            Y[r, fr.off[st[1]] + st[2]] = st[3]
    return Y


# ------------------------------------------------------------------------------------------------------------------------------- route --
def launch_list(fr, split=None, lds_maxd=1, lds=True, generic=False):
    """The work list tspws_build_inverse (csrc/inverse.hip) makes for this frame, restated from its documented rule: one item per run of
    scales with the same D (an octave), or one per scale when the octave items together have fewer than 768 waves (split: forces either
    form); items whose D divides N first; a wave = 64 lanes = up to 64 output phases x groups of 8 outputs.  Returns dict(items, per_scale,
    waves, waves_lds, waves_fast, generic) -- what tspws_hip_inverse_info must answer -- and body[s], chunks[s] per scale."""
    D, Ns, N, S = fr.D, fr.Ns, fr.N, fr.S

    def nwaves(d, ns):
        dl = 1
        while dl < d and dl < 64:
            dl <<= 1
        ng, gw = -(-ns // INV_R), 64 // dl
        return (-(-d // 64) if d > 64 else 1) * -(-ng // gw)

    runs, s = [], 0
    while s < S:
        e = s + 1
        while e < S and D[e] == D[s]:
            e += 1
        runs.append((s, e))
        s = e
    if split is None:
        split = sum(nwaves(int(D[a]), int(Ns[a])) for a, _ in runs) < 768
    items = [(s, s + 1) for s in range(S)] if split else runs
    items = sorted(items, key=lambda it: N % int(D[it[0]]) != 0)       # (stable: scale order inside a class)
    woff = wfast = wlds = 0
    for a, _ in items:
        gen = N % int(D[a]) != 0
        start = woff
        woff += nwaves(int(D[a]), int(Ns[a]))
        if not gen:
            wfast = woff
            if int(D[a]) <= lds_maxd and wlds == start:
                wlds = woff
    if not lds:
        wlds = 0
    per_scale = len(items) == S
    body, chunks = [], []
    for s in range(S):
        d = int(D[s])
        chunks.append(-(-d // 64) if d > 64 else 1)
        if generic:
            body.append("generic")
        elif N % d:
            body.append("GEN")
        elif lds and wlds and d <= lds_maxd:
            body.append("LDS-staged")
        elif d >= 64:
            body.append("wave-uniform")
        else:
            body.append("per-lane")
    return dict(items=len(items), per_scale=int(per_scale), waves=woff, waves_lds=wlds, waves_fast=wfast, generic=int(generic),
                body=body, chunks=chunks)


def body_of(s, route, row=None, nsets=None):
    """The kernel body scale s takes by the route (launch_list, checked against tspws_hip_inverse_info), for row `row` of a call with
    `nsets` sets: the LDS-staged form runs only for the paired sets of a call with two or more pairs."""
    if not route:
        return "body not known"
    if route.get("generic"):
        return "k_inverse_generic"
    b = route["body"][s]
    if b == "LDS-staged" and row is not None and nsets is not None and (nsets // 2 < 2 or row >= 2 * (nsets // 2)):
        b = "per-lane (LDS-staged in calls with two or more pairs)"
    if b == "wave-uniform":
        b += f", {route['chunks'][s]} chunk(s) of 64 phases"
    return "k_inv_poly " + b + (", one item per scale" if route["per_scale"] else ", one item per octave")


# ----------------------------------------------------------------------------------------------------------------------------- checker --
class InverseMismatch(AssertionError):
    """A sample outside its bound: .row, .scale (None for a row summed over all scales), .sample, .ratio."""

    def __init__(self, msg, row, scale, sample, ratio):
        super().__init__(msg)
        self.row, self.scale, self.sample, self.ratio = row, scale, sample, ratio


def check_rows(got, ref, rows=None, route=None, nsets=None):
    """|got[i] - want[rows[i]]| <= bound[rows[i]] at EVERY sample of every row (none left out; NaN fails).  rows: the reference rows the rows
    of `got` are (default: the first len(got)); nsets: sets of the call they come from (default len(got)).  Returns dict(ratio, row, scale,
    sample, by_kind): the worst |diff| / bound, where it occurs, and the worst per kind of set ("full" / "scale" / "impulse" / "zero")."""
    got = np.asarray(got)
    rows = list(range(got.shape[0])) if rows is None else list(rows)
    nsets = got.shape[0] if nsets is None else nsets
    assert got.ndim == 2 and got.shape == (len(rows), ref.N) and got.dtype == np.float64, (got.shape, got.dtype, len(rows), ref.N)
    want, bound = ref.want[rows], ref.bound[rows]
    diff = np.abs(got.astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0))
    ratio = np.where(np.isfinite(got), ratio, np.inf).astype(np.float64)      # NaN / inf: an unwritten or broken sample
    i, n = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    i, n = int(i), int(n)
    kind = ref.kinds[rows[i]]
    s = kind[1] if len(kind) > 1 else None
    worst = dict(ratio=float(ratio[i, n]), row=i, scale=s, sample=n, by_kind={})
    for j, rmax in enumerate(ratio.max(axis=1)):
        k = ref.kinds[rows[j]][0]
        worst["by_kind"][k] = max(worst["by_kind"].get(k, 0.0), float(rmax))
    nbad = int(np.count_nonzero(~(ratio <= 1.0)))
    if nbad:
        fr = ref.fr
        if s is None:
            where = f"a {kind[0]} set (sum over {fr.S} scales)"
        else:
            where = (f"{'impulse at k = %d of' % kind[2] if kind[0] == 'impulse' else 'single-scale set of'} scale {s} of {fr.S} (D = {int(fr.D[s])}, "
                     f"L = {int(fr.L[s])}, N_s = {int(fr.Ns[s])}; {body_of(s, route, i, nsets)})")
        raise InverseMismatch(
            f"{nbad} sample(s) outside the bound; worst in row {i} of a call with {nsets} set(s), {where}, sample {n} of {ref.N}: got {float(got[i, n])!r}, "
            f"want {float(want[i, n])!r}, |diff| / bound = {worst['ratio']:.3g} (bound {float(bound[i, n]):.3g})", i, s, n, worst["ratio"])
    return worst
