"""CPU-side checks of the stretching call (tspws_hip_stretch_rows, tspws_stretch_grid): the library exports the entry points and the binding
declares them; every refusal that needs no device, with a NULL plan, host dummies and sentinel-filled outputs unchanged; the grid rule; and
the checker's own tests (tests/stretch_rows_ref.py) -- it recovers a known stretch from analytically stretched rows, its bound holds for
FP64 evaluations in three summation orders, and it catches one float32 ulp in the reference and 1e-9 in a grid entry."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import stretch_rows_ref as srr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_stretch_rows", "tspws_hip_stretch_rows_stats", "tspws_stretch_grid")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("stretch_rows", "stretch_rows_stats"):
        assert hasattr(tspws.Plan, n), n
    assert callable(tspws.stretch_grid)
    stats = (C.c_uint * 5)()
    assert lib.tspws_hip_stretch_rows_stats(None, C.byref(stats)) == -1
    assert b"stretch_rows_stats: NULL" in lib.tspws_hip_last_error()


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------
def call(lib, rows=True, ref=True, eps=(-0.01, 0.0, 0.01), epsp=True, win=((3, 9), (0, 16)), winp=True, cc=True, fit=True, ld=256, ldr=256, z=7.5, B=2, M=3,
         E=None, W=None):
    """One tspws_hip_stretch_rows call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is
    refused before device work)."""
    d_rows, d_ref = np.full(16, 7.0, np.float32), np.full(16, 5.0, np.float32)
    o_cc, o_fit = np.full(64, -3.0), np.full(64, -4.0)
    e = np.array(eps, dtype=np.float64)
    w = np.array(win, dtype=np.uint64).reshape(-1)
    rc = lib.tspws_hip_stretch_rows(None, d_rows.ctypes.data if rows else None, ld, B, M, None, d_ref.ctypes.data if ref else None, ldr, z,
                                    e.ctypes.data if epsp else None, e.size if E is None else E, w.ctypes.data if winp else None, w.size // 2 if W is None else W,
                                    o_cc.ctypes.data if cc else None, o_fit.ctypes.data if fit else None, None)
    assert (o_cc == -3.0).all() and (o_fit == -4.0).all() and (d_rows == 7.0).all() and (d_ref == 5.0).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


def test_stretch_rows_refusals(lib):
    # the NULL plan itself, with everything else in order (also without a cc output, with B == 0 / M == 0, and with what only the plan can
    # judge: short strides and a window past max -- the NULL plan is what refuses them here)
    for kw in (dict(), dict(cc=False), dict(B=0), dict(M=0), dict(ld=3), dict(ldr=3), dict(win=((0, 10 ** 9),)), dict(z=-1e300), dict(eps=(0.5,)),
               dict(eps=(-0.5, 0.5)), dict(win=((0, 1), (0, 1), (0, 2), (1, 2)))):
        rc, err = call(lib, **kw)
        assert rc == -1 and b"stretch_rows: NULL" in err, (kw, err)
    for kw in (dict(rows=False), dict(ref=False), dict(epsp=False), dict(winp=False), dict(fit=False)):
        rc, err = call(lib, **kw)
        assert rc == -1 and b"stretch_rows: NULL" in err, (kw, err)
    # what needs no plan comes first
    for E in (0, 4097, 10 ** 6):
        rc, err = call(lib, E=E)
        assert rc == -1 and b"stretch_rows: 1 to 4096 stretch factors" in err, (E, err)
    for W in (0, 5, 100):
        rc, err = call(lib, W=W)
        assert rc == -1 and b"stretch_rows: 1 to 4 windows" in err, (W, err)
    for eps in ((0.0, 0.0), (0.01, 0.0), (-0.01, 0.01, 0.005)):
        rc, err = call(lib, eps=eps)
        assert rc == -1 and b"stretch_rows: the stretch factors must increase strictly" in err, (eps, err)
    for eps in ((float("nan"),), (0.0, float("nan")), (-0.6, 0.0), (0.0, 0.5000001), (float("inf"),)):
        rc, err = call(lib, eps=eps)
        assert rc == -1 and b"stretch_rows: a stretch factor that is NaN or outside" in err, (eps, err)
    for z in (float("nan"), float("inf"), -float("inf")):
        rc, err = call(lib, z=z)
        assert rc == -1 and b"stretch_rows: a NaN or infinite zero-lag position" in err, (z, err)
    for win in (((5, 5),), ((9, 3),), ((0, 4), (7, 7))):
        rc, err = call(lib, win=win)
        assert rc == -1 and b"stretch_rows: an empty window" in err, (win, err)


# ---- the grid rule ---------------------------------------------------------------------------------------------------------------------------
def test_stretch_grid(lib):
    for eps_max, E in ((0.01, 41), (0.01, 201), (0.5, 3), (0.03, 49), (1e-4, 4095)):
        g = tspws.stretch_grid(eps_max, E)
        h = (E - 1) // 2
        assert g.dtype == np.float64 and g.shape == (E,) and g[h] == 0.0 and not np.signbit(g[h])
        assert np.array_equal(g[:h].view(np.uint64) ^ np.uint64(1 << 63), g[::-1][:h].copy().view(np.uint64))  # symmetric bit for bit
        assert (np.diff(g) > 0).all() and g[-1] == np.float64(h) * (np.float64(eps_max) / np.float64(h))
        want = (np.arange(E, dtype=np.float64) - np.float64(h)) * (np.float64(eps_max) / np.float64(h))
        assert np.array_equal(g, want)
    buf = np.full(8, 9.0)
    fn = lib.tspws_stretch_grid
    assert fn(None, 0.01, 5) == 1
    for eps_max, E in ((0.01, 4), (0.01, 2), (0.01, 1), (0.01, 0), (0.0, 5), (-0.01, 5), (0.6, 5), (float("nan"), 5), (float("inf"), 5)):
        assert fn(buf.ctypes.data, eps_max, E) == 2, (eps_max, E)
    assert (buf == 9.0).all()  # nothing written
    assert fn(buf.ctypes.data, 0.5, 5) == 0 and buf[:5].tolist() == [-0.5, -0.25, 0.0, 0.25, 0.5] and (buf[5:] == 9.0).all()
    with pytest.raises(tspws.TspwsError):
        tspws.stretch_grid(0.01, 40)


# ---- the checker's own tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(lib):
    """Seed 0's analytic rows, the grid and the checker's answer: shared by the tests below, never changed."""
    eps = tspws.stretch_grid(0.01, 41)
    ref, rows = srr.analytic_rows(0)
    want = srr.reference(rows[None], ref[None], srr.Z, eps, srr.WINDOWS)
    return eps, ref, rows, want


def test_checker_recovers_the_stretch(case):
    eps, ref, rows, want = case
    step = eps[1] - eps[0]
    got = srr.fit(want["cc"][0].astype(np.float64), eps)
    for j, e0 in enumerate(srr.EPS0):
        for w in range(len(srr.WINDOWS)):
            eh, ch, es, edge = got[j, w]
            print(f"eps0 {e0:+.5f} window {srr.WINDOWS[w]}: eps_hat {eh:+.6f} ({abs(eh - e0) / step:.3f} of a step), cc_hat {ch:.5f}, e* {es:.0f}, edge {edge:.0f}")
            assert abs(eh - e0) <= step / 2 and ch >= 0.99 and edge == 0 and es == want["argmax"][0, j, w]
    assert srr.margins_ok(want)
    # eps = 0 reproduces the reference exactly: the unstretched row against itself correlates to 1 within the bound
    mid = (eps.size - 1) // 2
    assert (np.abs(want["cc"][0, 2, :, mid] - 1) <= want["b_cc"][0, 2, :, mid]).all()


def test_bound_holds_under_reordering_and_catches_a_change(case):
    eps, ref, rows, want = case
    for order in ("forward", "reversed", "pairwise"):
        srr.check(srr.fp64_cc(rows, ref, srr.Z, eps, srr.WINDOWS, order)[None], want, f"fp64 numpy, {order}")
    # one float32 ulp in one reference sample (inside all windows' reach), and 1e-9 in one grid entry: outside in at least one cc
    bad = ref.copy()
    bad[300] = np.nextafter(bad[300], np.float32(np.inf))
    with pytest.raises(AssertionError):
        srr.check(srr.fp64_cc(rows, bad, srr.Z, eps, srr.WINDOWS)[None], want, "one ulp of the reference")
    e2 = eps.copy()
    e2[7] += 1e-9
    with pytest.raises(AssertionError):
        srr.check(srr.fp64_cc(rows, ref, srr.Z, e2, srr.WINDOWS)[None], want, "1e-9 in a grid entry")
    # ... and the NaN rule: a dead row, a row left out
    r2 = rows.copy()
    r2[1] = 0
    w2 = srr.reference(r2[None], ref[None], srr.Z, eps, srr.WINDOWS, mtr=np.array([[1, 1, 0]], np.uint32))
    assert np.isnan(w2["cc"][0, 1:].astype(np.float64)).all() and (w2["argmax"][0, 1:] == -1).all() and not np.isnan(w2["cc"][0, 0].astype(np.float64)).any()
    f2 = srr.fit(w2["cc"][0].astype(np.float64), eps)
    assert np.isnan(f2[1:, :, :2]).all() and (f2[1:, :, 2] == -1).all() and (f2[1:, :, 3] == 1).all()
