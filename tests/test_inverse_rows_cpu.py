"""The per-scale reference of the inverse frame transform and its checker (tests/inverse_rows_ref.py) tested on the CPU.

* The reference agrees with the oracle (abi.OracleFrame.inverse, pinned to the reference's goldens) within the bound, on full sets, on
  single-scale sets and on impulses, for every case of tests/test_inverse_rows_gpu.py; the cap max b_s / max |x_s| < 1e-12 holds for each.
* Rows that carry one defect IN ONE SCALE are rejected, with the scale named.  For each defect the test also evaluates the check the suite had
  before -- one global relerr(x, x_oracle) < 1e-11 on the sum over scales -- and asserts what it does with it:

      admitted by the global check, rejected here:  a tap in the filter's flank rounded to float32 (coarse scale); one wrapped tap term of the
                                                    first coefficient dropped next to the circular seam; one scale wrong by 1e-9 of its size
      rejected by both:                             the coefficient window of one output phase shifted by one row; the rows of two sets
                                                    swapped; one scale missing altogether; a NaN sample

  The mutation data is white noise under an amplitude envelope that dips to 1e-5 at the seam -- the dynamic range of a weighted plane: on
  flat white noise the smallest wrapped term is ~2e-9 of the row maximum, which the global check catches; under the envelope it is ~1e-14 of
  the row maximum and only a bound that follows the local coefficients sees it.  This is what shows, without a GPU, that
  tests/test_inverse_rows_gpu.py fails when a kernel is subtly wrong in one scale."""
import numpy as np
import pytest

import abi
import inverse_rows_engine as eng
from inverse_rows_ref import CAP, TOL64, Frame, InverseMismatch, assemble, body_of, check_rows, launch_list, reference_rows, scale_rows


def frame_of(c):
    return Frame.from_oracle(abi.resolve(abi.default_params(**c["kw"]), c["N"]), c["N"])


@pytest.mark.parametrize("c", eng.CASES, ids=[eng.name_of(c) for c in eng.CASES])
def test_reference_agrees_with_the_oracle_and_the_cap_holds(c):
    fr = frame_of(c)
    sets, Y, ref = eng.reference_of(c, fr)
    assert 0 < ref.cap_ratio < CAP == TOL64 / 10
    kinds = {k[0] for k in ref.kinds}
    assert kinds == {"full", "scale", "impulse"} and sum(k[0] == "scale" for k in ref.kinds) == fr.S
    rows = list(range(len(sets))) if c["N"] <= 4097 else list(range(0, len(sets), 3))      # (the long frame: every third row, 30 in all)
    xo = np.stack([fr.oracle.inverse(Y[r]) for r in rows])
    w = check_rows(xo, ref, rows=rows, route=launch_list(fr))
    assert 0 < w["ratio"] <= 1
    # today's global check agrees on the full sets, and the single-scale rows add up to row 0
    assert abi.relerr(xo[0], ref.want[0].astype(np.float64)) < 1e-14
    if c["N"] <= 4097:
        F = c["F"]
        assert abi.relerr(xo[F: F + fr.S].sum(axis=0), xo[0]) < 1e-13


def test_launch_list_restates_the_documented_rule():
    """Known lists: the default frame at N = 32768 is the first with 768 octave waves (one item per octave, 12 items); N = 4096 has one item
    per scale; Mexican hat N = 2048 stages its four D = 1 scales (4 waves each); N = 4097 has only three-frame items."""
    r = launch_list(frame_of(eng.CASES[9]))
    assert (r["items"], r["per_scale"], r["waves"], r["waves_lds"], r["waves_fast"]) == (12, 0, 768, 0, 768)
    r = launch_list(frame_of(eng.CASES[0]))
    assert (r["items"], r["per_scale"], r["waves"], r["waves_lds"], r["waves_fast"]) == (36, 1, 288, 0, 288)
    assert body_of(0, r) == "k_inv_poly per-lane, one item per scale" and "wave-uniform, 8 chunk(s)" in body_of(35, r)
    fr = frame_of(eng.CASES[4])
    r = launch_list(fr)
    assert (r["items"], r["waves"], r["waves_lds"], r["waves_fast"]) == (14, 56, 16, 56) and r["body"][:5] == ["LDS-staged"] * 4 + ["per-lane"]
    assert "LDS-staged" in body_of(0, r, row=1, nsets=4) and body_of(0, r, row=2, nsets=3).startswith("k_inv_poly per-lane (LDS-staged in calls")
    assert launch_list(fr, lds=False)["waves_lds"] == 0 and launch_list(fr, lds_maxd=32)["waves_lds"] == 56
    assert launch_list(fr, split=False)["items"] == 6 and launch_list(fr, generic=True)["body"][0] == "generic"
    r = launch_list(frame_of(eng.CASES[1]))
    assert r["waves_fast"] == 0 and set(r["body"]) == {"GEN"} and "GEN" in body_of(3, r)


# ------------------------------------------------------------------------------------------------------------------------------ defects --
@pytest.fixture(scope="module", params=[(dict(), 4096), (dict(), 4097)], ids=lambda c: f"N={c[1]}")
def case(request):
    """Two full sets under the envelope, then the S single-scale sets of the first; the oracle's rows of all of them."""
    kw, N = request.param
    fr = frame_of(dict(kw=kw, N=N))
    rng = np.random.default_rng(N)
    env = np.concatenate([1e-5 + np.sin(np.pi * np.arange(fr.Ns[s]) * fr.D[s] / N) ** 2 for s in range(fr.S)])
    full = [(rng.standard_normal(fr.ncoef) + 1j * rng.standard_normal(fr.ncoef)) * env for _ in range(2)]
    sets = [("full", y) for y in full] + [("scale", s, full[0][fr.off[s]: fr.off[s + 1]].copy()) for s in range(fr.S)]
    ref = reference_rows(fr, sets)
    xo = np.stack([fr.oracle.inverse(y) for y in assemble(fr, sets)])
    check_rows(xo, ref)
    return dict(fr=fr, ref=ref, xo=xo, y0=full[0], route=launch_list(fr))


def part(c, s):
    return c["y0"][c["fr"].off[s]: c["fr"].off[s + 1]]


def verdicts(c, s, delta):
    """The oracle's rows with `delta` added to scale s's share -- in the single-scale row and in full row 0.  Both must be rejected here (the
    single-scale one with its scale named); returns whether the global check on the sum over scales admits the full row."""
    xo, ref = c["xo"], c["ref"]
    got = xo.copy()
    got[0] += delta
    got[2 + s] += delta
    with pytest.raises(InverseMismatch) as e:
        check_rows(got[2 + s: 3 + s], ref, rows=[2 + s], route=c["route"])
    assert e.value.scale == s and f"scale {s} of" in str(e.value) and f"D = {int(c['fr'].D[s])}, L = {int(c['fr'].L[s])}" in str(e.value), str(e.value)
    assert body_of(s, c["route"], 0, 1) in str(e.value)
    with pytest.raises(InverseMismatch) as e:
        check_rows(got[:2], ref, route=c["route"])
    assert e.value.row == 0 and e.value.scale is None and e.value.ratio > 1
    return bool(abi.relerr(got[0], xo[0]) < TOL64)


def as64(x):
    return np.asarray(x, np.float64)


@pytest.mark.parametrize("s", [1, 21])
def test_a_wrapped_tap_term_dropped_next_to_the_seam(case, s):
    """The term of the first coefficient and the last tap -- raw position cd - (L - 1) < 0, i.e. across the circular seam -- missing from one
    output of one scale (D = 2; D = 64): the global check admits it."""
    fr = case["fr"]
    L, cd, D = int(fr.L[s]), int(fr.cd[s]), int(fr.D[s])
    w, y = fr.wd[fr.toff[s] + L - 1], part(case, s)[0]
    delta = np.zeros(fr.N)
    assert cd - (L - 1) < 0
    delta[(cd - (L - 1)) % fr.N] = -float(fr.gain[s]) * D * (w.real * y.real + w.imag * y.imag)
    assert verdicts(case, s, delta) is True


@pytest.mark.parametrize("s", [22, 30])
def test_a_tap_rounded_to_float32(case, s):
    """One tap three scale lengths off the centre of a coarse scale's filter (D = 64; D = 256) rounded to float32: the global check admits it."""
    fr = case["fr"]
    wd = fr.wd[fr.toff[s]: fr.toff[s + 1]].copy()
    l0 = int(fr.L[s]) // 2 + int(3 * fr.scale[s])
    wd[l0] = np.complex64(wd[l0])
    assert wd[l0] != fr.wd[fr.toff[s] + l0]
    delta = as64(scale_rows(fr, s, part(case, s), wd)[0][0] - scale_rows(fr, s, part(case, s))[0][0])
    assert verdicts(case, s, delta) is True


def test_one_scale_wrong_at_the_1e9_level_or_missing(case):
    """The scale with the smallest share of the row maximum (under 1e-2 of it), wrong by 1e-9 of its size: the global check admits it.  Missing
    altogether, neither check admits it -- nor a 1e-9 error in a scale with a large share."""
    xo, S = case["xo"], case["fr"].S
    share = np.abs(xo[2: 2 + S]).max(axis=1) / np.abs(xo[0]).max()
    s = int(np.argmin(share))
    assert share[s] < 1e-2 and share[5] > 1e-1
    assert verdicts(case, s, -1e-9 * xo[2 + s]) is True
    assert verdicts(case, s, -xo[2 + s]) is False
    assert verdicts(case, 5, -1e-9 * xo[2 + 5]) is False


@pytest.mark.parametrize("s", [2, 24])
def test_the_window_of_one_output_phase_shifted_by_one_row(case, s):
    """The outputs of ONE phase of the decimation grid (n - cd = 1 mod D) computed from the coefficient row one further on."""
    fr = case["fr"]
    D, cd = int(fr.D[s]), int(fr.cd[s])
    shifted = as64(scale_rows(fr, s, np.roll(part(case, s), -1))[0][0])
    phase = (np.arange(fr.N) - cd) % D == 1
    delta = np.where(phase, shifted - case["xo"][2 + s], 0.0)
    assert verdicts(case, s, delta) is False


def test_rows_of_two_sets_swapped(case):
    got = case["xo"][:2][::-1].copy()
    with pytest.raises(InverseMismatch) as e:
        check_rows(got, case["ref"])
    assert e.value.ratio > 1e6 and not abi.relerr(got[0], case["xo"][0]) < TOL64


def test_a_nan_sample_is_rejected(case):
    for row, scale in ((0, None), (2 + 7, 7)):
        got = case["xo"].copy()
        got[row, 100] = np.nan
        with pytest.raises(InverseMismatch) as e:
            check_rows(got, case["ref"])
        assert (e.value.row, e.value.scale, e.value.sample) == (row, scale, 100) and e.value.ratio == np.inf
        assert not abi.relerr(got[0], case["xo"][0]) < TOL64 or row


def test_zero_rows_and_impulses_have_exact_supports(case):
    """A zero set has zero bound: any non-zero sample is rejected; outside an impulse's L outputs the bound is zero too."""
    fr = case["fr"]
    s = 20
    ref = reference_rows(fr, [("zero",), ("impulse", s, int(fr.Ns[s]) - 1, complex(0, -0.75))])
    got = ref.want.astype(np.float64)
    assert not got[0].any() and np.count_nonzero(ref.bound[1]) <= int(fr.L[s]) and check_rows(got, ref)["ratio"] <= 0.25
    xo = fr.oracle.inverse(assemble(fr, [("impulse", s, int(fr.Ns[s]) - 1, complex(0, -0.75))])[0])
    assert check_rows(np.stack([got[0], xo]), ref)["ratio"] <= 1
    for row in (0, 1):
        bad = got.copy()
        bad[row, int(np.flatnonzero(ref.bound[1] == 0)[0])] = 1e-300
        with pytest.raises(InverseMismatch):
            check_rows(bad, ref)
