"""CPU reference for the band rows (tspws_hip_inverse_bands, Plan.inverse_bands), with a bound at every output sample, the frames, coefficient
sets and band tables of tests/test_band_rows_gpu.py, and the checker that holds device rows to the reference (the checker itself is tested
in tests/test_band_rows_cpu.py).  No GPU import here.

For a coefficient set Y and a band [s_begin, s_end) of a frame:

    X = sum_{s in band} x_s(Y)          x_s = inverse_rows_ref.scale_rows: scale s's share of the inverse, in np.longdouble
    Q = sum_{s in band} x_s(-i Y)       -i Y = (Im Y, -Re Y): the quadrature comes from the SAME function on the rotated set

and the bound at every sample has no number of its own:

    bound[n] = sum_{s in band} b_s[n] + n_band 2^-52 sum_{s in band} |x_s[n]|

with b_s = (2 T_s + 6) 2^-52 B_s of inverse_rows_ref (the dot product of scale s in any order) and the second term for the combining kernel's
n_band additions.  An empty band is a zero row with a zero bound.  inverse_rows_ref's CAP holds for the rotated sets too: scale_shares asserts
max_n b_s / max_n |x_s| < 1e-12 for every scale of every set AND of every rotated set, so no sample meets a loose bound."""
import numpy as np

from inverse_rows_ref import CAP, EPS, LD, Frame, scale_rows  # noqa: F401  (Frame: for the callers)


def rotate(Y):
    """-i Y = (Im Y, -Re Y), without a rounding."""
    Y = np.asarray(Y, np.complex128)
    Z = np.empty_like(Y)
    Z.real, Z.imag = Y.imag, -Y.real
    return Z


class Shares:
    """x[s], b[s] (longdouble [2 nset][N]: the sets, then the rotated sets) of the scales asked for, and the cap ratio over them."""

    def __init__(self, fr, Y):
        self.fr, self.Y = fr, np.atleast_2d(np.asarray(Y, np.complex128))
        self.nset = self.Y.shape[0]
        self.both = np.concatenate([self.Y, rotate(self.Y)])
        self.x, self.b = {}, {}
        self.cap_ratio = 0.0

    def scale(self, s):
        if s not in self.x:
            fr = self.fr
            x, B = scale_rows(fr, s, self.both[:, fr.off[s]: fr.off[s + 1]])
            b = (2 * int(fr.T[s]) + 6) * EPS * B
            mx = np.abs(x).max(axis=1)
            assert (mx > 0).all(), f"scale {s}: a set without data in this scale has no cap ratio -- give it other data"
            ratio = float((b.max(axis=1) / mx).max())
            assert ratio < CAP, (f"scale {s} (D = {int(fr.D[s])}, L = {int(fr.L[s])}, N_s = {int(fr.Ns[s])}): max b_s / max |x_s| = {ratio:.3g} is not "
                                 f"below {CAP:g} for a set or a rotated set: give the case other data, not a wider cap")
            self.cap_ratio = max(self.cap_ratio, ratio)
            self.x[s], self.b[s] = x, b
        return self.x[s], self.b[s]


class BandRef:
    """want / bound [2][nset][R][N] longdouble: index 0 the real rows X, 1 the quadrature Q."""

    def __init__(self, fr, bands, want, bound, cap_ratio):
        self.fr, self.bands, self.want, self.bound, self.cap_ratio = fr, [tuple(int(v) for v in b) for b in bands], want, bound, cap_ratio
        _, self.nset, self.R, self.N = want.shape


def reference_bands(fr, Y, bands, shares=None):
    """The reference of the sets Y[nset][ncoef] and the table `bands`.  `shares`: a Shares of the same frame and sets, kept between calls."""
    sh = Shares(fr, Y) if shares is None else shares
    nset, N, R = sh.nset, fr.N, len(bands)
    want, bound = np.zeros((2, nset, R, N), LD), np.zeros((2, nset, R, N), LD)
    for r, (a, e) in enumerate(bands):
        a, e = int(a), int(e)
        assert 0 <= a <= e <= fr.S
        sum_abs = np.zeros((2 * nset, N), LD)
        w, bd = np.zeros((2 * nset, N), LD), np.zeros((2 * nset, N), LD)
        for s in range(a, e):
            x, b = sh.scale(s)
            w += x
            bd += b
            sum_abs += np.abs(x)
        bd += (e - a) * EPS * sum_abs
        want[0, :, r], want[1, :, r] = w[:nset], w[nset:]
        bound[0, :, r], bound[1, :, r] = bd[:nset], bd[nset:]
    return BandRef(fr, bands, want, bound, sh.cap_ratio)


class BandMismatch(AssertionError):
    pass


def check_bands(got, ref, part=0, sets=None, bands=None, extra=None):
    """|got - want| <= bound at EVERY sample of every row (none left out; NaN fails).  got[nset'][R'][N] float64; part 0: real rows, 1:
    quadrature; sets / bands: the reference's sets / bands the rows of `got` are (default: the first nset' / all); extra: a second bound
    [nset'][R'][N] added to the reference's (rows of another route, held to the sum of the two bounds).  Returns the worst |diff| / bound."""
    got = np.asarray(got)
    sets = list(range(got.shape[0])) if sets is None else list(sets)
    bands = list(range(ref.R)) if bands is None else list(bands)
    assert got.dtype == np.float64 and got.shape == (len(sets), len(bands), ref.N), (got.dtype, got.shape, len(sets), len(bands), ref.N)
    want, bound = ref.want[part][np.ix_(sets, bands)], ref.bound[part][np.ix_(sets, bands)]
    if extra is not None:
        bound = bound + extra
    diff = np.abs(got.astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0))
    ratio = np.where(np.isfinite(got), ratio, np.inf).astype(np.float64)
    nbad = int(np.count_nonzero(~(ratio <= 1.0)))
    worst = float(ratio.max()) if ratio.size else 0.0
    if nbad:
        j, r, n = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        a, e = ref.bands[bands[r]]
        raise BandMismatch(f"{nbad} sample(s) outside the bound; worst in the {'quadrature' if part else 'real'} row of set {sets[j]}, band {bands[r]} = "
                           f"[{a}, {e}) of {ref.fr.S} scales, sample {n} of {ref.N}: got {float(got[j, r, n])!r}, want {float(want[j, r, n])!r}, "
                           f"|diff| / bound = {worst:.3g} (bound {float(bound[j, r, n]):.3g})")
    return worst


# ------------------------------------------------------------------------------------------------ the GPU cases (tests/test_band_rows_gpu.py) --
def gpu_cases():
    """(case of inverse_rows_engine.CASES, set counts of the runs): the smallest frame that reaches each kernel body."""
    import inverse_rows_engine as ire
    want = [
        (dict(), 4096, (1, 2, 5)),               # baseline: per-lane and wave-uniform scales
        (dict(), 4097, (1, 2, 5)),               # GEN form
        (dict(b0=3.0), 3072, (1, 2, 5)),         # idle phases
        (dict(type=-3), 2048, (1, 2, 5)),        # D = 1 LDS-staged form (2 or more pairs of sets; with the quadrature: 2 or more sets)
        (dict(b0=0.25), 4096, (1, 2, 5)),        # LDS-staged form, several blocks of tap steps
        (dict(J=2), 64, (1, 2, 5)),              # smallest frame
        (dict(), 32768, (1, 2)),                 # D > 64 wave-uniform chunks
    ]
    out = []
    for kw, N, counts in want:
        hit = [c for c in ire.CASES if c["kw"] == kw and c["N"] == N]
        assert len(hit) == 1, (kw, N)
        out.append((hit[0], counts))
    return out


def case_id(c):
    return f"N{c['N']}-" + ("-".join(f"{k}{v}" for k, v in c["kw"].items()) or "default")


def band_sets(c, fr, nset):
    """nset full coefficient sets, seeded by the case: white complex-normal, each with one stretch of exact zeros inside one scale and one
    subnormal (every scale of every set keeps data: the cap ratio needs it)."""
    rng = np.random.default_rng(1000 + c["seed"])
    Y = rng.standard_normal((nset, fr.ncoef)) + 1j * rng.standard_normal((nset, fr.ncoef))
    for i in range(nset):
        sz = (fr.S // 2 + i) % fr.S
        if int(fr.Ns[sz]) >= 8:
            a = int(fr.off[sz]) + int(fr.Ns[sz]) // 3
            Y[i, a: a + max(1, int(fr.Ns[sz]) // 4)] = 0
        Y[i, int(fr.off[i % fr.S]) + 1] = complex(1e-310, 0)
    return Y


def band_table(S, V):
    """Every single scale, [0, S), an empty band, two overlapping bands that cut octaves between voices, the last scale alone."""
    t = [(s, s + 1) for s in range(S)]
    t += [(0, S), (min(3, S), min(3, S)), (min(1, S), min(V + 2, S)), (min(max(V, 1) - 1, S), min(2 * V + 1, S)), (S - 1, S)]
    return t
