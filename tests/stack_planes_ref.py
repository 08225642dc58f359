"""CPU reference for the two FP64 planes every output of the library is made of -- the linear stack ST = sum_t Y_t and the phase stack
PS = sum_t Y_t / |Y_t| (reference ts_pws1f_lib.c:486-494) -- with a per-coefficient error bound, and the checker that holds device planes
to it (tests/test_stack_planes_gpu.py; the checker itself is tested in tests/test_stack_planes_cpu.py).  No GPU import here.

The coefficients come from the oracle (abi.OracleFrame.forward, pinned to the reference's goldens by tests/test_oracle_vs_golden.py); moduli,
phasors and all four sums are formed in np.longdouble, trace by trace (never [M][ncoef]).

The bounds use no number of their own.  The suite already holds the device's per-trace coefficients of scale s to
d[t,s] = TOL64 * max_k |Y_t,s[k]|, TOL64 = 1e-11 (test_hip_parity.py::test_forward_inverse_vs_oracle, scale by scale).  For coefficient k of
scale s of an ensemble of M traces:

    bST[k] = sum_t d[t,s]  +  M * 2^-52 * sum_t |Y_t[k]|                                  (coefficient tolerance + any summation order)
    bPS[k] = sum_t ( Y_t[k] == 0 ? 0 : min(2, d[t,s] / |Y_t[k]|) )  +  M * 2^-50

(|u(y + e) - u(y)| <= |e| / |y| to first order for the phasor u(y) = y / |y|; two unit phasors differ by at most 2; a zero coefficient adds
nothing on either side.)  A bound that is too loose would hide a failure, so reference_planes asserts max bPS < 1e-6 for an ensemble without
stretches of zeros and < 1e-2 for one with the suite's usual holes: a wrong or missing phasor (an error of order 1) is then at least 1e6
(1e2) times over the limit wherever it lands."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import abi

TOL64 = 1e-11
CAP_PLAIN = 1e-6     # max bPS of an ensemble without zero stretches (an all-zero trace is allowed: its terms are 0)
CAP_HOLES = 1e-2     # ... of one with the usual holes
LD = np.longdouble
CLD = np.clongdouble


def punch_holes(X):
    """The suite's usual holes (tests/spectral_engine.py): an all-zero trace, a stretch of exact zeros longer than most filters, a zero head."""
    M, N = X.shape
    X[M // 3] = 0
    X[M // 2, N // 4: N // 2] = 0
    X[M - 1, : N // 8] = 0
    return X


class PlaneRef:
    """ST, PS, bST, bPS (float64 / complex128 arrays of ncoef), the scale offsets off[S + 1] and the frame tables D, L, Ns."""

    def __init__(self, ST, PS, bST, bPS, off, D, L, Ns, M, N, holes):
        self.ST, self.PS, self.bST, self.bPS, self.off = ST, PS, bST, bPS, off
        self.D, self.L, self.Ns, self.M, self.N, self.holes = D, L, Ns, M, N, holes
        self.S = len(D)
        self.max_bPS = float(bPS.max())
        self.cap = CAP_HOLES if holes else CAP_PLAIN

    def scale_of(self, i):
        return int(np.searchsorted(self.off, i, side="right") - 1)


def _workers():
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def reference_planes(params, N, X, holes=False):
    """Reference planes and bounds of the rows X[M][N] (float32 or float64) for the RESOLVED parameter set `params`.
    holes: X carries stretches of exact zeros (punch_holes) -- the cap on max bPS is 1e-2 instead of 1e-6."""
    X = np.asarray(X)
    assert X.ndim == 2 and X.shape[1] == N and X.dtype in (np.float32, np.float64)
    M = X.shape[0]
    f = abi.OracleFrame.from_params(params, N)
    nc, S = f.ncoef, f.S
    Ns = f.Ns.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
    assert off[-1] == nc
    ST, PS = np.zeros(nc, CLD), np.zeros(nc, CLD)
    sum_abs, sum_d, ph = np.zeros(nc, LD), np.zeros(nc, LD), np.zeros(nc, LD)
    two = LD(2)
    nw = _workers()
    with ThreadPoolExecutor(nw) as pool:       # (orc_forward runs outside the GIL; the sums stay in trace order)
        for t0 in range(0, M, nw):
            for Y in pool.map(lambda t: f.forward(X[t].astype(np.float64)), range(t0, min(M, t0 + nw))):
                Yl = Y.astype(CLD)
                mag = np.abs(Yl)
                nz = Y != 0                                # exactly: the reference's 0 / 0 is skipped (ts_pws1f_lib.c:489-492)
                if not nz.any():
                    continue
                safe = np.where(nz, mag, LD(1))
                d = LD(TOL64) * np.repeat(np.maximum.reduceat(mag, off[:-1]), Ns)    # d[t,s] at every coefficient of scale s
                ST += Yl
                PS += np.where(nz, Yl / safe, 0)
                sum_abs += mag
                sum_d += d
                ph += np.where(nz, np.minimum(two, d / safe), 0)
    bST = (sum_d + LD(M) * LD(2.0 ** -52) * sum_abs).astype(np.float64)
    bPS = (ph + LD(M) * LD(2.0 ** -50)).astype(np.float64)
    ref = PlaneRef(ST.astype(np.complex128), PS.astype(np.complex128), bST, bPS, off, f.D.astype(np.int64), f.L.astype(np.int64), Ns, M, N, holes)
    assert ref.max_bPS < ref.cap, f"max bPS = {ref.max_bPS:.3g} is not below {ref.cap:g} ({M} x {N}, holes={holes}): give the case other data, not a wider cap"
    return ref


def engine_of(s, route):
    """Which forward engine scale s of a many-trace call belongs to; route = dict(S, spec_first, spec_end, many) from
    tspws_hip_spectral_choice / tspws_hip_spectral_end_scale (None: not known)."""
    if not route:
        return "engine not known"
    if route["spec_first"] < route["S"]:
        if route["spec_first"] <= s < route["spec_end"]:
            return "spectral chain"
        if s >= route["spec_end"]:
            return "clipped scale: k_fwd_gemm contraction"
        return "k_fwd_tl / k_fwd_poly beside the spectral chain"
    return "k_fwd_tl / k_fwd_poly (trace-lane path)" if route.get("many") else "k_fwd_lds / k_fwd_poly (few-trace kernels)"


class PlaneMismatch(AssertionError):
    """A coefficient outside its bound: .plane ("ST" / "PS"), .scale, .index (within the scale), .ratio."""

    def __init__(self, msg, plane, scale, index, ratio):
        super().__init__(msg)
        self.plane, self.scale, self.index, self.ratio = plane, scale, index, ratio


def _worst(got, want, bound):
    diff = np.abs(np.asarray(got, np.complex128) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
    ratio = np.where(np.isfinite(diff), ratio, np.inf)     # NaN / inf: an unwritten or broken coefficient
    i = int(np.argmax(ratio))
    return float(ratio[i]), i, int(np.count_nonzero(~(ratio <= 1.0)))


def check_planes(ST, PS, ref, route=None):
    """|ST - ref.ST| <= bST and |PS - ref.PS| <= bPS at EVERY coefficient (none left out; NaN fails).  Returns
    dict(rST, sST, iST, rPS, sPS, iPS): the worst ratios |dST| / bST, |dPS| / bPS with the scale and the index in it where they occur."""
    assert ST.shape == ref.ST.shape and PS.shape == ref.PS.shape, (ST.shape, PS.shape, ref.ST.shape)
    out = {}
    bad = None
    for plane, got, want, bound in (("ST", ST, ref.ST, ref.bST), ("PS", PS, ref.PS, ref.bPS)):
        r, i, nbad = _worst(got, want, bound)
        s = ref.scale_of(i)
        k = i - int(ref.off[s])
        out["r" + plane], out["s" + plane], out["i" + plane] = r, s, k
        if nbad and (bad is None or r > bad[1]):
            bad = (plane, r, s, k, i, nbad, got, want, bound)
    if bad:
        plane, r, s, k, i, nbad, got, want, bound = bad
        raise PlaneMismatch(
            f"{plane}: {nbad} coefficient(s) outside the bound; worst at scale {s} of {ref.S} (D = {int(ref.D[s])}, L = {int(ref.L[s])}, N_s = {int(ref.Ns[s])}; "
            f"{engine_of(s, route)}), index {k}: got {complex(got[i])!r}, want {complex(want[i])!r}, |diff| / bound = {r:.3g} (bound {bound[i]:.3g}); "
            f"{ref.M} x {ref.N}", plane, s, k, r)
    return out
