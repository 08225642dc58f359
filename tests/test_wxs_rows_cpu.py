"""CPU-side checks of the wavelet cross-spectrum calls (tspws_hip_wxs_coef, tspws_hip_wxs_rows): the library exports the entry points and
the binding declares them; every refusal that needs no device, with a NULL plan, host dummies and sentinel-filled outputs unchanged; and the
checker's own tests (tests/wxs_rows_ref.py) on coefficient sets of the oracle's forward transform: plain FP64 evaluations in two different
orders lie inside its bounds, a deliberately wrong term is caught, the parity inputs hold no term whose phase FP64 rounding could flip
between +pi and -pi and none whose participation is undecided, and the recovery input gives back its stretch with the sign of the contract."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import abi
import wxs_rows_ref as wr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_wxs_coef", "tspws_hip_wxs_rows", "tspws_hip_wxs_rows_stats")
SEED = 0  # the parity inputs: the first seed without flip or undecided terms (test_parity_inputs_decide_every_term holds it to that)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("wxs_coef", "wxs_rows", "wxs_rows_stats", "forward"):
        assert hasattr(tspws.Plan, n), n
    stats = (C.c_uint * 5)()
    assert lib.tspws_hip_wxs_rows_stats(None, C.byref(stats)) == -1
    assert b"wxs_rows_stats: NULL" in lib.tspws_hip_last_error()


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------
def call(lib, coef, a=True, b=True, bands=((0, 2), (1, 1)), bandp=True, win=((3, 9), (0, 16)), winp=True, sums=True, fit=True, z=7.5, R=None, W=None, **kw):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    x, y = np.full(16, 7.0), np.full(16, 5.0)
    o_sums, o_fit = np.full(64, -3.0), np.full(64, -4.0)
    bt = np.array(bands, dtype=np.uint32).reshape(-1)
    w = np.array(win, dtype=np.uint64).reshape(-1)
    R, W = bt.size // 2 if R is None else R, w.size // 2 if W is None else W
    tail = (z, bt.ctypes.data if bandp else None, R, w.ctypes.data if winp else None, W, 0, o_sums.ctypes.data if sums else None,
            o_fit.ctypes.data if fit else None, None)
    if coef:
        rc = lib.tspws_hip_wxs_coef(None, x.ctypes.data if a else None, y.ctypes.data if b else None, None, kw.get("nrow", 2), kw.get("B", 2), *tail)
    else:
        rc = lib.tspws_hip_wxs_rows(None, x.ctypes.data if a else None, kw.get("ld", 256), kw.get("B", 2), kw.get("M", 3), None, y.ctypes.data if b else None,
                                    kw.get("ldr", 256), *tail)
    assert (o_sums == -3.0).all() and (o_fit == -4.0).all() and (x == 7.0).all() and (y == 5.0).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


@pytest.mark.parametrize("coef", (True, False))
def test_refusals_without_a_plan(lib, coef):
    who = b"wxs_coef: " if coef else b"wxs_rows: "
    # the NULL plan itself, with everything else in order (also without sums, empty, and with what only the plan can judge)
    for kw in (dict(), dict(sums=False), dict(B=0), dict(M=0), dict(nrow=0), dict(ld=3), dict(ldr=3), dict(win=((0, 10 ** 9),)), dict(bands=((0, 10 ** 6),)),
               dict(z=-1e300), dict(nrow=5)):
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + b"NULL" in err, (kw, err)
    for kw in (dict(a=False), dict(b=False), dict(bandp=False), dict(winp=False), dict(fit=False)):
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + b"NULL" in err, (kw, err)
    for kw, text in ((dict(R=0), b"1 to 64 bands"), (dict(R=65), b"1 to 64 bands"), (dict(W=0), b"1 to 4 windows"), (dict(W=5), b"1 to 4 windows"),
                     (dict(bands=((0, 2), (3, 2))), b"a band with s_begin > s_end"), (dict(win=((3, 9), (5, 5))), b"an empty window (n0 >= n1)"),
                     (dict(win=((9, 3),)), b"an empty window (n0 >= n1)"), (dict(z=float("nan")), b"a NaN or infinite zero-lag position"),
                     (dict(z=float("-inf")), b"a NaN or infinite zero-lag position")):
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + text in err, (kw, err)


# ---- the checker's own tests ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    return wr.Frame.from_oracle(abi.resolve(abi.default_params(), wr.N), wr.N)


def oracle_sets(fr, rows, ref):
    """(Yc [B M][ncoef], Yr [B][ncoef], ens) of a parity batch through the oracle's forward transform."""
    B, M = rows.shape[:2]
    Yc = np.stack([fr.oracle.forward(rows[b, m, :fr.N].astype(np.float64)) for b in range(B) for m in range(M)])
    Yr = np.stack([fr.oracle.forward(ref[b, :fr.N].astype(np.float64)) for b in range(B)])
    return Yc, Yr, np.arange(B * M, dtype=np.uint32) // M


@pytest.fixture(scope="module")
def sets(frame):
    rows, ref, _ = wr.parity_batch(SEED)
    return oracle_sets(frame, rows, ref)


def test_parity_inputs_decide_every_term(frame, sets):
    Yc, Yr, ens = sets
    bands = wr.parity_bands(frame)
    for z in wr.ZS:
        for skip in (False, True):
            w = wr.reference(frame, Yc, Yr, z, bands, wr.WINDOWS, ens=ens, skip_wrapped=skip)
            assert w["flips"] == 0 and w["undecided"] == 0, (z, skip, w["flips"], w["undecided"])
            live = w["sums"][..., 1] > 0
            rel = (w["b_sums"][live][:, 1:] / np.abs(w["sums"][live][:, 1:7]).max()).astype(np.float64)
            assert np.isfinite(w["b_sums"].astype(np.float64)).all()
            print(f"z = {z}, skip_wrapped = {skip}: rows x windows x bands with terms {int(live.sum())}, largest bound / largest |sum| {rel.max():.3g}")
    # the all-zero row and the reference that is zero inside window 0 give sums without terms where no filter reaches a non-zero sample
    w = wr.reference(frame, Yc, Yr, wr.Z, bands, wr.WINDOWS, ens=ens)
    assert (w["sums"][5] == 0).all() and (w["sums"][:, :, 4] == 0).all()  # (the empty band)
    assert (w["sums"][9:18, 0, :4, 0] < w["sums"][:9, 0, :4, 0].max(axis=0)).all()


@pytest.mark.parametrize("order", ("forward", "pairwise", "reversed"))
def test_fp64_orders_lie_inside_the_bounds(frame, sets, order):
    Yc, Yr, ens = sets
    bands = wr.parity_bands(frame)
    for i in (0, 4, 13, 24):
        for skip in (False, True):
            want = wr.reference(frame, Yc[i:i + 1], Yr[ens[i]:ens[i] + 1], 750.25, bands, wr.WINDOWS, skip_wrapped=skip)
            got = wr.fp64_sums(frame, Yc[i], Yr[ens[i]], 750.25, bands, wr.WINDOWS, skip_wrapped=skip, order=order)
            wr.check(got[None], want, f"row {i} {order} skip {skip}")


def test_a_wrong_term_is_caught(frame, sets):
    Yc, Yr, ens = sets
    bands = wr.parity_bands(frame)
    want = wr.reference(frame, Yc[:1], Yr[:1], wr.Z, bands, wr.WINDOWS)
    good = wr.fp64_sums(frame, Yc[0], Yr[0], wr.Z, bands, wr.WINDOWS)
    wr.check(good[None], want, "as it should be")
    # ONE of the ~2000 terms of band 0 with the opposite phase
    bad = wr.fp64_sums(frame, Yc[0], Yr[0], wr.Z, bands, wr.WINDOWS, wrong=(5, 100))
    assert not np.array_equal(bad, good)
    with pytest.raises(AssertionError, match="outside its bound"):
        wr.check(bad[None], want, "one wrong phase")
    # one term dropped from a sum: n is no longer exact
    bad = good.copy()
    bad[2, 0, 0] -= 1
    with pytest.raises(AssertionError, match="n differs"):
        wr.check(bad[None], want, "one term missing")
    # a NaN where the checker has none
    bad = good.copy()
    bad[1, 1, 3] = np.nan
    with pytest.raises(AssertionError, match="NaN positions"):
        wr.check(bad[None], want, "a NaN")


def test_fit_of_the_contract():
    # a line delta = 2e-3 t + 0.5 with unit weights: the slope, the intercept, no residual; and the degenerate cases
    t = np.arange(-8.0, 9.0)
    d = 2e-3 * t + 0.5
    s = np.array([t.size, t.size, t.sum(), (t * t).sum(), d.sum(), (t * d).sum(), (d * d).sum(), 3.0, 4.0])
    f = wr.fit(s)
    assert abs(f[0] - 2e-3) < 1e-15 and abs(f[1] - 0.5) < 1e-13 and f[3] < 1e-6 and f[4] == 5.0 / t.size and f[5] == t.size
    assert wr.cr_hypot(3.0, 4.0) == 5.0 and wr.cr_hypot(1e-200, 1e-200) == np.sqrt(2.0) * 1e-200 and wr.cr_hypot(0.0, 0.0) == 0.0
    one = np.array([1, 2.0, 6.0, 18.0, 1.0, 3.0, 0.5, 0.0, 2.0])       # one term: no slope
    f = wr.fit(one)
    assert np.isnan(f[:4]).all() and f[4] == 1.0 and f[5] == 1
    f = wr.fit(np.zeros(9))                                           # no term: coh is 0 / 0
    assert np.isnan(f[:5]).all() and f[5] == 0
    f = wr.fit(np.full(9, np.nan))                                    # a row left out
    assert np.isnan(f[:5]).all() and f[5] == -1


def test_recovery_input():
    """The checker's own estimate on the recovery input: eps_hat within 10 % of eps = 2e-3, in the contract's sign, and coh > 0.9."""
    fr = wr.Frame.from_oracle(abi.resolve(abi.default_params(), wr.RN), wr.RN)
    ref, row = wr.recovery_rows()
    band = wr.recovery_band(fr)
    assert (fr.omega[band[0][0]:band[0][1]] * wr.REPS * max(abs(n - wr.RZ) for n in wr.RWIN[0])).max() < np.pi / 2
    Yr, Yc = fr.oracle.forward(ref.astype(np.float64))[None], fr.oracle.forward(row.astype(np.float64))[None]
    for skip in (False, True):
        w = wr.reference(fr, Yc, Yr, wr.RZ, band, wr.RWIN, skip_wrapped=skip)
        f = wr.fit(w["sums"].astype(np.float64))[0, 0, 0]
        print(f"skip_wrapped = {skip}: eps_hat {f[0]:.6e}, icpt {f[1]:+.4f}, err {f[2]:.3g}, rms {f[3]:.3g}, coh {f[4]:.4f}, n {f[5]:.0f}")
        assert w["flips"] == 0 and w["undecided"] == 0
        assert abs(f[0] - wr.REPS) <= 0.1 * wr.REPS and f[4] > 0.9
