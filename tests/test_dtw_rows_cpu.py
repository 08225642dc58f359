"""The checker of the dynamic time warping call (tests/dtw_rows_ref.py) against itself, on the CPU: the dynamic programme against the brute
force over every admissible path on tiny cases whose errors are small dyadic numbers (all sums exact, so equality is exact); the tie rule;
the clamp at both trace ends; the range of one sample; dead rows; the fit formula against np.polyfit in longdouble; the parity batch's seed."""
import numpy as np
import pytest

import dtw_rows_ref as dr


def dyadic_case(rng, n, Lmax, pad=4):
    """(c, r float32 [1][n + 2 pad], n0, n1): multiples of 1/8 with both maxima exactly 1, so ac = ar = 1 and every e is a multiple of 1/64."""
    Nn = n + 2 * pad
    c = rng.integers(-8, 9, (1, Nn)).astype(np.float32) / 8
    r = rng.integers(-8, 9, (1, Nn)).astype(np.float32) / 8
    c[0, pad] = 1.0
    r[0, pad] = -1.0
    return c, r, pad, pad + n


@pytest.mark.parametrize("b", (1, 2, 3))
@pytest.mark.parametrize("Lmax", (1, 2))
def test_dp_equals_brute_force(b, Lmax):
    rng = np.random.default_rng(100 * b + Lmax)
    for n in (2, 3, 5, 7, 9):
        for _ in range(3 if n == 9 else 6):
            c, r, n0, n1 = dyadic_case(rng, n, Lmax)
            o = dr.dtw(c, r, n0, n1, Lmax, b, 3.5)
            e = o["e"][0]
            assert (e * 64 == np.round(e * 64)).all() and not o["dead"][0]
            best, arg = dr.brute(e, b)
            assert o["D_end"][0].min() == best                                   # the minimum, exactly
            path = o["lag"][0]
            assert dr.admissible(path, b, Lmax)
            assert tuple(int(v) + Lmax for v in path) in arg                     # the backtracked path attains it
            assert sum(e[i, path[i] + Lmax] for i in range(n)) == best
            assert o["fit"][0, 4] == best / n


def test_tie_rule_prefers_centre_then_minus_then_first_lag():
    # a reference that is constant makes every lag equal: all candidates tie everywhere
    c = np.array([[0.5, 1.0, -0.25, 0.75, 0.5, 0.25, 1.0, 0.5]], np.float32)
    r = np.ones((1, 8), np.float32)
    o = dr.dtw(c, r, 0, 8, 2, 1, 0.0)
    assert o["ties"][0] == 7
    ch = o["choice"][0]
    assert (ch[1:] == dr.C_).all()                    # dc <= dm && dc <= dp wins a tie
    assert (o["lag"][0] == -2).all()                  # the first smallest D_end in ascending l
    assert o["fit"][0, 5] == 8 and o["fit"][0, 0] == 0.0
    # dm == dp < dc: Mn.  Two samples, lags -1 .. 1: e[0] = (1, 4, 1) / 4, so at l = 0 the slanted candidates tie below the centre one
    e = np.array([[[0.25, 1.0, 0.25], [0.0, 0.0, 0.0]]])
    D_end, ch, ties = dr.accumulate(e, 1)
    assert ch[0, 1, 1] == dr.MN and ties[0] == 1 and ch[0, 1, 0] == dr.C_ and ch[0, 1, 2] == dr.C_


def test_clamp_at_both_trace_ends():
    rng = np.random.default_rng(5)
    c = rng.integers(-8, 9, (1, 12)).astype(np.float32) / 8
    r = rng.integers(-8, 9, (1, 12)).astype(np.float32) / 8
    c[0, 3], r[0, 7] = 1.0, 1.0
    e, dead = dr.errors(c, r, 0, 12, 3)
    assert not dead[0]
    for i in range(12):
        for li, l in enumerate(range(-3, 4)):
            k = min(max(i + l, 0), 11)
            assert e[0, i, li] == (np.float64(c[0, i]) - np.float64(r[0, k])) ** 2
    assert (e[0, 0, :3] == e[0, 0, 3]).all() and (e[0, 11, 4:] == e[0, 11, 3]).all()   # the nearest in-range error


def test_range_of_one_sample():
    c = np.array([[0.0, 0.5, 0.0, 0.0]], np.float32)
    r = np.array([[0.25, 0.0, 1.0, 0.5]], np.float32)
    o = dr.dtw(c, r, 1, 2, 2, 3, 0.0)
    # e = (1 - r[clamp(1 + l)])^2 over l = -2 .. 2 = r[0], r[0], r[1], r[2], r[3]
    assert np.array_equal(o["e"][0, 0], [0.5625, 0.5625, 1.0, 0.0, 0.25])
    assert o["lag"][0].tolist() == [1]
    f = o["fit"][0]
    assert np.isnan(f[:3]).all() and f[3] == 0.0 and f[4] == 0.0 and f[5] == 0.0
    o = dr.dtw(c, r, 1, 2, 1, 3, 0.0)
    assert o["lag"][0].tolist() == [1] and o["fit"][0, 5] == 1.0 and np.isnan(o["fit"][0, 0])


def test_dead_rows():
    rng = np.random.default_rng(9)
    c = rng.standard_normal((6, 40)).astype(np.float32)
    r = rng.standard_normal((6, 40)).astype(np.float32)
    c[0, 10:20] = 0                     # mc == 0
    r[1, 7:23] = 0                      # mr == 0 over the reach [10 - 3, 20 + 3)
    c[2, 15] = np.nan
    r[3, 22] = np.nan                   # inside the reach, outside the range
    c[4, 12] = np.inf
    r[5, 23] = np.nan                   # just outside the reach: alive
    o = dr.dtw(c, r, 10, 20, 3, 2, 0.0)
    assert o["dead"].tolist() == [True, True, True, True, True, False]
    assert np.isnan(o["fit"][:5, :5]).all() and (o["fit"][:5, 5] == -1).all() and (o["lag"][:5] == dr.INT_MIN).all()
    assert np.isfinite(o["fit"][5]).all() and (np.abs(o["lag"][5]) <= 3).all()


def test_fit_against_polyfit_in_longdouble():
    rng = np.random.default_rng(11)
    for n, Lmax, n0, z in ((600, 10, 800, 750.0), (1501, 127, 0, 750.25), (37, 5, 3, 0.0), (2, 1, 7, 1e3)):
        steps = rng.integers(-1, 2, (8, n))
        lag = np.clip(np.cumsum(steps, axis=1), -Lmax, Lmax)
        fit = dr.fit_of(lag, np.full(8, 3.0), n0, z, Lmax)
        t = (np.arange(n0, n0 + n) - np.longdouble(z))
        for k in range(8):
            y = lag[k].astype(np.longdouble)
            tm = t.mean()
            slope = ((t - tm) * (y - y.mean())).sum() / ((t - tm) ** 2).sum()
            icpt = y.mean() - slope * tm
            assert np.allclose(np.polyfit((t - tm).astype(np.float64), lag[k].astype(np.float64), 1)[0], float(slope), rtol=1e-9, atol=1e-12)
            res = y - (icpt + slope * t)
            rms = np.sqrt((res ** 2).mean())
            assert abs(fit[k, 0] - float(slope)) <= 1e-9 * max(abs(float(slope)), 1e-3)
            assert abs(fit[k, 1] - float(icpt)) <= 1e-9 * max(abs(float(icpt)), 1.0)
            assert abs(fit[k, 3] - float(rms)) <= 1e-6 * max(float(rms), 1e-3)
            assert abs(fit[k, 2] - float(rms / np.sqrt(((t - tm) ** 2).sum()))) <= 1e-6 * max(fit[k, 2], 1e-6)
            assert fit[k, 4] == 3.0 / n and fit[k, 5] == (np.abs(lag[k]) == Lmax).sum()


def test_recovery_by_the_checker():
    tol, eh = dr.recovery_tolerance()
    assert (np.sign(eh[0]) == 1).all() and (np.sign(eh[1]) == -1).all()
    assert (np.abs(np.abs(eh) - dr.REPS) < 0.1 * dr.REPS).all(), eh     # the method finds eps to a tenth on this input


def test_a_seed_is_well_posed():
    assert any(dr.well_posed(seed) for seed in range(3))
