"""The plane-level checker (tests/stack_planes_ref.py) tested on the CPU: planes that carry one of the defects the float32 metric of the
suite lets through (or nearly: max|a-b| / max|b| < 2e-6 after weighting and the inverse transform) must be REJECTED, with the right
scale named; planes rebuilt from coefficients perturbed at rounding level (<= 1e-13 relative -- summation order, device
libm), summed in plain float64 in another order, must PASS with room.  This is what shows, without a GPU, that
tests/test_stack_planes_gpu.py fails when a kernel is subtly wrong."""
import numpy as np
import pytest

import abi
from stack_planes_ref import PlaneMismatch, check_planes, punch_holes, reference_planes

SHAPES = [(dict(), 130, 4097), (dict(unbiased=1), 96, 16501)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: f"{c[1]}x{c[2]}")
def case(request):
    kw, M, N = request.param
    X = abi.synth_traces(M, N, seed=41)
    X[M // 3] = 0
    p = abi.resolve(abi.default_params(**kw), N)
    ref = reference_planes(p, N, X)
    f = abi.OracleFrame.from_params(p, N)
    Ys = [f.forward(x.astype(np.float64)) for x in X]      # (test only: the reference itself never holds [M][ncoef])
    return dict(M=M, N=N, X=X, ref=ref, Ys=Ys, rng=np.random.default_rng(1000 + M))


def unit(Y):
    mag = np.abs(Y)
    return np.where(mag > 0, Y / np.where(mag > 0, mag, 1.0), 0.0)


def rejected(c, ST, PS, plane=None, scales=None):
    with pytest.raises(PlaneMismatch) as e:
        check_planes(ST, PS, c["ref"])
    if plane is not None:
        assert e.value.plane == plane, str(e.value)
    if scales is not None:
        assert e.value.scale in scales and f"scale {e.value.scale} of" in str(e.value), str(e.value)
    assert e.value.ratio > 1e2, str(e.value)               # (every one of these defects lies 1e2 .. 3e8 times over the limit)
    return e.value


def test_the_reference_passes_its_own_check(case):
    r = check_planes(case["ref"].ST, case["ref"].PS, case["ref"])
    assert r["rST"] == 0 and r["rPS"] == 0
    assert case["ref"].max_bPS < 1e-6


@pytest.mark.parametrize("up", [0, 4])
def test_a_trace_missing_from_the_phase_stack_of_one_scale(case, up):
    """One trace's phasors missing from the coarsest scale (a k_fwd_gemm scale at these lengths) / from the scale four above it."""
    ref = case["ref"]
    s = ref.S - 1 - up
    a, b = int(ref.off[s]), int(ref.off[s + 1])
    t = int(case["rng"].integers(0, case["M"] // 3))
    PS = ref.PS.copy()
    PS[a:b] -= unit(case["Ys"][t][a:b])
    rejected(case, ref.ST, PS, "PS", {s})


@pytest.mark.parametrize("which", ["coarse", "scale10"])
def test_one_phasor_missing_at_one_coefficient(case, which):
    ref = case["ref"]
    s = ref.S - 3 if which == "coarse" else 10
    if which == "scale10":
        assert int(ref.D[10]) == 8
    k = int(case["rng"].integers(0, ref.Ns[s]))
    t = case["M"] - 2
    PS = ref.PS.copy()
    PS[int(ref.off[s]) + k] -= unit(case["Ys"][t])[int(ref.off[s]) + k]
    e = rejected(case, ref.ST, PS, "PS", {s})
    assert e.index == k


def test_last_trace_of_a_partial_block_counted_twice(case):
    """... in the four coarsest scales, both planes."""
    ref = case["ref"]
    a = int(ref.off[ref.S - 4])
    Y = case["Ys"][case["M"] - 1]
    ST, PS = ref.ST.copy(), ref.PS.copy()
    ST[a:] += Y[a:]
    PS[a:] += unit(Y)[a:]
    rejected(case, ST, PS, None, set(range(ref.S - 4, ref.S)))
    rejected(case, ref.ST, PS, "PS", set(range(ref.S - 4, ref.S)))
    rejected(case, ST, ref.PS, "ST", set(range(ref.S - 4, ref.S)))


def test_phasors_normalised_in_float32(case):
    """A float reciprocal square root in the phase normalisation: 25 times under the float metric, far over the plane bound."""
    ref = case["ref"]
    PS = np.zeros_like(ref.PS)
    for Y in case["Ys"]:
        r2 = (Y.real * Y.real + Y.imag * Y.imag).astype(np.float32)
        inv = np.where(r2 > 0, np.float32(1) / np.sqrt(np.where(r2 > 0, r2, np.float32(1))), np.float32(0)).astype(np.float64)
        PS += Y * inv
    rejected(case, ref.ST, PS, "PS")


def test_coefficients_rounded_to_float32(case):
    """A float intermediate in front of BOTH stacks (per-scale ST error ~4e-8): each plane is rejected on its own."""
    ref = case["ref"]
    ST, PS = np.zeros_like(ref.ST), np.zeros_like(ref.PS)
    for Y in case["Ys"]:
        Yf = Y.astype(np.complex64).astype(np.complex128)
        ST += Yf
        PS += unit(Yf)
    rejected(case, ST, ref.PS, "ST")
    rejected(case, ref.ST, PS, "PS")


@pytest.mark.parametrize("order", ["forward", "reversed", "blocks of 64"])
def test_rounding_level_differences_pass(case, order):
    """Coefficients perturbed by 1e-13 of each (trace, scale) maximum -- every one by the full amount, in a random direction -- and summed in
    plain float64, in trace order, reversed, and in 64-trace blocks like the many-trace kernels: both ratios stay below 0.1."""
    ref, M = case["ref"], case["M"]
    rng = np.random.default_rng(7)
    off = ref.off

    def perturbed(t):
        Y = case["Ys"][t]
        mx = np.repeat(np.maximum.reduceat(np.abs(Y), off[:-1]), ref.Ns)
        return np.where(Y != 0, Y + 1e-13 * mx * np.exp(2j * np.pi * rng.uniform(size=Y.size)), 0.0)

    Yp = [perturbed(t) for t in range(M)]
    idx = list(range(M))[::-1] if order == "reversed" else list(range(M))
    ST, PS = np.zeros_like(ref.ST), np.zeros_like(ref.PS)
    if order == "blocks of 64":
        for b0 in range(0, M, 64):
            st, ps = np.zeros_like(ST), np.zeros_like(PS)
            for t in idx[b0: b0 + 64]:
                st += Yp[t]
                ps += unit(Yp[t])
            ST += st
            PS += ps
    else:
        for t in idx:
            ST += Yp[t]
            PS += unit(Yp[t])
    r = check_planes(ST, PS, ref)
    assert 0 < r["rST"] < 0.1 and 0 < r["rPS"] < 0.1, r


def test_unwritten_and_nan_coefficients_are_rejected(case):
    ref = case["ref"]
    for plane in ("ST", "PS"):
        P = {"ST": ref.ST.copy(), "PS": ref.PS.copy()}
        i = int(ref.off[5]) + 3
        P[plane][i] = complex(np.nan, np.nan)
        with pytest.raises(PlaneMismatch) as e:
            check_planes(P["ST"], P["PS"], ref)
        assert e.value.plane == plane and e.value.scale == 5 and e.value.index == 3


def test_caps_on_the_bound_are_conditions():
    """An ensemble with stretches of zeros does not fit the 1e-6 cap (coefficients at a hole's edge are tiny: their phasors are ill
    conditioned) and is refused unless it is declared; declared, it fits 1e-2.  An all-zero ensemble has zero planes and zero ST bound."""
    M, N = 40, 2048
    p = abi.resolve(abi.default_params(), N)
    X = punch_holes(abi.synth_traces(M, N, seed=3))
    with pytest.raises(AssertionError):
        reference_planes(p, N, X)
    ref = reference_planes(p, N, X, holes=True)
    assert 1e-6 < ref.max_bPS < 1e-2
    z = reference_planes(p, N, np.zeros((3, N), np.float32))
    assert not z.ST.any() and not z.PS.any() and not z.bST.any()
    check_planes(z.ST, z.PS, z)
    ST = z.ST.copy()
    ST[7] = 1e-300
    with pytest.raises(PlaneMismatch):
        check_planes(ST, z.PS, z)


def test_the_message_names_the_engine_of_the_scale(case):
    """With the route of a many-trace call (tspws_hip_spectral_choice / tspws_hip_spectral_end_scale) the message says which engine the failing
    scale belongs to: trace-lane kernel below the spectral set, the chain inside it, the contraction behind it."""
    ref = case["ref"]
    S = ref.S
    route = dict(S=S, spec_first=16, spec_end=S - 5, many=True)
    for s, word in ((3, "k_fwd_tl"), (20, "spectral chain"), (S - 2, "k_fwd_gemm")):
        PS = ref.PS.copy()
        PS[int(ref.off[s])] += 1.0
        with pytest.raises(PlaneMismatch, match=word) as e:
            check_planes(ref.ST, PS, ref, route)
        assert e.value.scale == s and f"D = {int(ref.D[s])}, L = {int(ref.L[s])}" in str(e.value)
    PS = ref.PS.copy()
    PS[0] += 1.0
    with pytest.raises(PlaneMismatch, match="few-trace kernels"):
        check_planes(ref.ST, PS, ref, dict(S=S, spec_first=S, spec_end=S, many=False))
