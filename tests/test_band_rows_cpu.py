"""CPU-side checks of the band rows (tspws_hip_inverse_bands, tspws_hip_stack_batch_bands, tspws_bands_from_frequencies): the library exports
the entry points and the binding declares them; every refusal that needs no device, with sentinel-filled outputs unchanged; the host rule
against a numpy restatement on the oracle's scale tables; and the checker's own tests (tests/band_rows_ref.py): a partition of [0, S) adds up
to inverse_rows_ref.reference_rows' full row within the two bounds, the quadrature of Y is the real row of -i Y, and the CAP holds for the sets
and the rotated sets of every case of tests/test_band_rows_gpu.py, so that no GPU test can meet a loose bound."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import abi
import band_rows_ref as brr
import inverse_rows_ref as irr

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_inverse_bands", "tspws_hip_stack_batch_bands", "tspws_hip_stack_batch_bands_stats", "tspws_bands_from_frequencies")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def test_entry_points(lib):
    with open(os.path.join(tspws.ROOT, "include", "tspws_hip.h")) as fh:
        header = fh.read()
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS and n + "(" in header, n
    for n in ("inverse_bands", "stack_batch_bands", "stack_batch_bands_stats"):
        assert hasattr(tspws.Plan, n), n
    assert hasattr(tspws, "bands_from_frequencies")
    stats = (C.c_uint * 9)()
    assert lib.tspws_hip_stack_batch_bands_stats(None, C.byref(stats)) == -1
    assert b"stack_batch_bands_stats: NULL" in lib.tspws_hip_last_error()


# ---- refusals: a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work) ----------
def inverse_bands(lib, bands=((0, 1), (1, 3)), R=None, Y=True, table=True, re=True, im=True, nset=2):
    bt = tspws.band_table(bands)
    R = bt.shape[0] if R is None else R
    dummy = np.full(16, 7.0, np.float64)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_inverse_bands(None, ptr(Y, dummy), nset, ptr(table, bt), R, ptr(re, dummy), ptr(im, dummy), None)
    assert (dummy == 7.0).all()
    return rc, lib.tspws_hip_last_error()


def stack_bands(lib, bands=((0, 1), (1, 3)), R=None, p=True, first=(0, 6, 9), table=True, ls=True, ts=True, ls_env=True, ts_env=True, x=True, ld=256, B=None):
    bt = tspws.band_table(bands)
    R = bt.shape[0] if R is None else R
    f = np.array(first, dtype=np.uint64) if first is not None else None
    B = (f.size - 1 if f is not None else 2) if B is None else B
    pp = abi.default_params()
    dummy = np.full(16, 7.0, np.float32)
    ptr = lambda on, a: a.ctypes.data if on else None  # noqa: E731
    rc = lib.tspws_hip_stack_batch_bands(None, C.byref(pp) if p else None, ptr(x, dummy), ld, ptr(f is not None, f) if f is not None else None, B,
                                         ptr(table, bt), R, ptr(ls, dummy), ptr(ts, dummy), ptr(ls_env, dummy), ptr(ts_env, dummy), None)
    assert (dummy == 7.0).all()
    return rc, lib.tspws_hip_last_error()


def test_inverse_bands_refusals(lib):
    for kw in (dict(), dict(Y=False), dict(table=False), dict(re=False), dict(im=False), dict(R=0), dict(nset=0)):  # (NULL plan in all of them)
        rc, err = inverse_bands(lib, **kw)
        assert rc == -1 and b"inverse_bands: NULL" in err, (kw, err)
    for bands in (((2, 1),), ((0, 1), (5, 4)), ((0, 0), (1, 1), (0xFFFFFFFF, 0))):
        rc, err = inverse_bands(lib, bands=bands)
        assert rc == -1 and b"inverse_bands: a band with s_begin > s_end" in err, (bands, err)
    for kw in (dict(R=1025), dict(R=1025, table=False), dict(R=0xFFFFFFFF, table=False)):
        rc, err = inverse_bands(lib, **kw)
        assert rc == -1 and b"inverse_bands: more than 1024 bands" in err, (kw, err)
    # 1024 bands are allowed: the NULL plan is what refuses them here (s_end > S needs the plan: tests/test_band_rows_gpu.py)
    rc, err = inverse_bands(lib, bands=[(0, 1)] * 1024)
    assert rc == -1 and b"inverse_bands: NULL" in err, err


def test_stack_batch_bands_refusals(lib):
    for kw in (dict(), dict(p=False), dict(first=None), dict(table=False), dict(ls=False), dict(ts=False), dict(x=False), dict(ld=3), dict(B=0), dict(R=0),
               dict(ls_env=False, ts_env=False)):
        rc, err = stack_bands(lib, **kw)
        assert rc == -1 and b"stack_batch_bands: NULL" in err, (kw, err)
    for kw in (dict(ls_env=False), dict(ts_env=False)):
        rc, err = stack_bands(lib, **kw)
        assert rc == -1 and b"stack_batch_bands: the two envelope outputs" in err, (kw, err)
    rc, err = stack_bands(lib, first=(0, 8, 6))
    assert rc == -1 and b"stack_batch_bands: decreasing" in err, err
    rc, err = stack_bands(lib, bands=((0, 1), (3, 2)))
    assert rc == -1 and b"stack_batch_bands: a band with s_begin > s_end" in err, err
    rc, err = stack_bands(lib, R=1025, table=False)
    assert rc == -1 and b"stack_batch_bands: more than 1024 bands" in err, err


# ---- the host rule --------------------------------------------------------------------------------------------------------------------------------
FRAMES = [(dict(), 16501), (dict(w0=2 * math.pi), 4096), (dict(type=-3), 2048)]


def oracle_scales(kw, N, dt):
    p = abi.resolve(abi.default_params(**kw), N, dt)
    return abi.OracleFrame.from_params(p, N).scale.copy(), float(p.w0)


def bands_numpy(scale, w0, dt, lo, hi):
    fc = np.array([w0 / (2 * tspws_pi() * dt * s) for s in scale])
    out = []
    for a, b in zip(lo, hi):
        idx = [s for s in range(len(scale)) if a <= fc[s] < b]
        assert idx == list(range(idx[0], idx[-1] + 1)) if idx else True
        if idx:
            out.append((idx[0], idx[-1] + 1))
        else:           # empty: at the first scale below the band (fc decreases with s)
            k = int(np.count_nonzero(fc >= b))
            out.append((k, k))
    return np.array(out, np.uint32).reshape(-1, 2), fc


def tspws_pi():
    return 3.14159265358979328


@pytest.mark.parametrize("kw,N", FRAMES, ids=["morlet-16501", "w0-2pi-4096", "mexhat-2048"])
@pytest.mark.parametrize("dt", [1.0, 0.05])
def test_bands_from_frequencies(lib, kw, N, dt):
    scale, w0 = oracle_scales(kw, N, dt)
    S = len(scale)
    fc0 = w0 / (2 * tspws_pi() * dt * scale)
    assert (np.diff(fc0) < 0).all()
    # edges between centre frequencies (geometric means: none closer than 1e-9 relative to a centre), below and above all scales
    mid = np.sqrt(fc0[:-1] * fc0[1:])
    edges = np.concatenate([[fc0[-1] * 0.25, fc0[-1] * 0.5], mid[::-3][:6][::-1] if S > 18 else mid[::-1], [fc0[0] * 2, fc0[0] * 4]])
    edges = np.unique(edges)
    assert min(abs(e / f - 1) for e in edges for f in fc0) > 1e-9
    bands, fc = tspws.bands_from_frequencies((scale, w0), dt, edges)
    want, fcw = bands_numpy(scale, w0, dt, edges[:-1], edges[1:])
    assert fc.tobytes() == fcw.tobytes() == fc0.tobytes()
    assert np.array_equal(bands, want), (bands, want)
    # shared edges partition the scales: bands come lowest frequency first, so they tile [0, S) from the back
    assert bands[0].tolist() == [S, S] and bands[-1].tolist() == [0, 0]       # below / above all scales: empty
    assert bands[-2, 0] == 0 and bands[1, 1] == S
    assert all(bands[r, 0] == bands[r + 1, 1] for r in range(len(bands) - 1))
    assert sum(int(e - a) for a, e in bands) == S
    # pairs: overlapping and nested bands, an edge pair with f_lo == f_hi (empty)
    pairs = np.array([[edges[1], edges[-2]], [edges[2], edges[3]], [edges[2], edges[2]], [edges[0], edges[-1]]])
    b2, _ = tspws.bands_from_frequencies(dict(scale=scale, w0=w0), dt, pairs)
    w2, _ = bands_numpy(scale, w0, dt, pairs[:, 0], pairs[:, 1])
    assert np.array_equal(b2, w2) and b2[0].tolist() == [0, S] and b2[3].tolist() == [0, S] and b2[2, 0] == b2[2, 1]
    # an edge exactly on a centre frequency: f_lo <= fc < f_hi
    k = S // 2
    b3, _ = tspws.bands_from_frequencies((scale, w0), dt, [[fc0[k], fc0[k - 1]], [fc0[k + 1], fc0[k]]])
    assert b3.tolist() == [[k, k + 1], [k + 1, k + 1 + 1]]


def test_bands_from_frequencies_refusals(lib):
    scale = np.array([2.0, 4.0, 8.0])
    lo, hi = np.array([0.1, 0.2]), np.array([0.2, 0.4])
    out = np.full((2, 2), 77, np.uint32)
    fc = np.full(3, 7.0)

    def call(scale=scale, dt=1.0, lo=lo, hi=hi, bands=out):
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        rc = lib.tspws_bands_from_frequencies(ptr(scale), 3, 6.0, dt, ptr(lo), ptr(hi), 2, ptr(bands), fc.ctypes.data)
        assert (out == 77).all() and (fc == 7.0).all()
        return rc, lib.tspws_hip_last_error()

    for kw in (dict(scale=None), dict(lo=None), dict(hi=None), dict(bands=None)):
        rc, err = call(**kw)
        assert rc == -1 and b"bands_from_frequencies: NULL" in err, (kw, err)
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        rc, err = call(dt=dt)
        assert rc == -1 and b"bands_from_frequencies: dt" in err, (dt, err)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for which in ("lo", "hi"):
            a = dict(lo=lo.copy(), hi=hi.copy())
            a[which][1] = bad
            rc, err = call(**a)
            assert rc == -1 and b"bands_from_frequencies: a band edge is not finite" in err, (bad, which, err)
    rc, err = call(lo=np.array([0.1, 0.5]))
    assert rc == -1 and b"bands_from_frequencies: f_lo > f_hi" in err, err
    with pytest.raises(tspws.TspwsError):
        tspws.bands_from_frequencies((scale, 6.0), 1.0, [0.3, 0.2])
    # fc may be NULL
    assert lib.tspws_bands_from_frequencies(scale.ctypes.data, 3, 6.0, 1.0, lo.ctypes.data, hi.ctypes.data, 2, out.ctypes.data, None) == 0
    assert not (out == 77).any()


# ---- the checker's own tests ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """A GEN frame (N = 4097 is large for a CPU test of its own; N = 515 has the same three-frame geometry) and three sets."""
    N = 515
    p = abi.resolve(abi.default_params(J=4), N)
    fr = irr.Frame.from_oracle(p, N)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((3, fr.ncoef)) + 1j * rng.standard_normal((3, fr.ncoef))
    return fr, Y, brr.Shares(fr, Y)


def test_partition_adds_up(small):
    fr, Y, sh = small
    S, V = fr.S, fr.V
    cuts = [0, 1, V + 2, 2 * V + 1, S]                   # cuts octaves between voices
    table = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)] + [(0, S), (2, 2)]
    ref = brr.reference_bands(fr, Y, table, sh)
    full = irr.reference_rows(fr, [("full", y) for y in Y])
    parts, pb = ref.want[0][:, :4].sum(axis=1), ref.bound[0][:, :4].sum(axis=1)
    assert (np.abs(parts - full.want) <= pb + full.bound).all()
    assert (np.abs(ref.want[0][:, 4] - full.want) <= ref.bound[0][:, 4] + full.bound).all()
    assert (ref.bound[0][:, 4] <= full.bound * (1 + 1e-15)).all() and (ref.bound[0][:, 4] > 0).all()  # [0, S): the full row's own bound
    assert not ref.want[:, :, 5].any() and not ref.bound[:, :, 5].any()                                 # the empty band
    # ... and the oracle's inverse agrees with the full band to the suite's FP64 tolerance
    for j in range(len(Y)):
        assert abi.relerr(ref.want[0][j, 4].astype(np.float64), fr.oracle.inverse(Y[j])) < irr.TOL64


def test_quadrature_is_real_row_of_rotated_set(small):
    fr, Y, sh = small
    table = [(0, fr.S), (1, fr.V + 2), (fr.S - 1, fr.S)]
    ref = brr.reference_bands(fr, Y, table, sh)
    rot = brr.reference_bands(fr, brr.rotate(Y), table)
    assert np.array_equal(ref.want[1], rot.want[0]) and np.array_equal(ref.bound[1], rot.bound[0])
    assert np.array_equal(rot.want[1], -ref.want[0])      # -i (-i Y) = -Y
    # check_bands holds rows to it: the reference itself passes, one sample one bound off fails, a NaN fails
    got = ref.want[1].astype(np.float64)
    assert brr.check_bands(got, ref, 1) <= 1
    bad = got.copy()
    bad[1, 2, 7] += 3 * float(ref.bound[1][1, 2, 7]) + 1e-300
    with pytest.raises(brr.BandMismatch):
        brr.check_bands(bad, ref, 1)
    bad = got.copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(brr.BandMismatch):
        brr.check_bands(bad, ref, 1)


CASES = brr.gpu_cases()


@pytest.mark.parametrize("c,counts", CASES, ids=[brr.case_id(c) for c, _ in CASES])
def test_cap_of_gpu_cases(c, counts):
    """Every scale of every set and of every rotated set of the GPU cases stays under the CAP (the oracle's taps here, the device's there:
    tests/test_hip_parity.py holds them to 1e-14 of each other)."""
    N = c["N"]
    fr = irr.Frame.from_oracle(abi.resolve(abi.default_params(**c["kw"]), N), N)
    sh = brr.Shares(fr, brr.band_sets(c, fr, max(counts)))
    for s in range(fr.S):
        sh.scale(s)
    assert 0 < sh.cap_ratio < brr.CAP
    table = brr.band_table(fr.S, fr.V)
    assert len(table) == fr.S + 5 and all(0 <= a <= e <= fr.S for a, e in table) and (0, fr.S) in table
    assert any(a == e for a, e in table) and table[-1] == (fr.S - 1, fr.S)


# ---- the batched call's checker (tests/band_batch_ref.py) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(unbiased=1), dict(unbiased=1, Kmax=4), dict(type=-3, wu=1.3)], ids=["biased", "unbiased", "kmax4", "mexhat-wu1.3"])
def test_batch_checker_against_oracle(kw):
    """The band [0, S) of the numpy definition is the oracle's tspws_main on the ensemble bit for bit (single- and two-stage ensembles); two
    bands that partition the scales add up to it to float rounding; an envelope is never below its row; empty ensemble and band: zero rows."""
    import band_batch_ref as bbr
    N = 1501
    p = abi.resolve(abi.default_params(**kw), N)
    X = abi.synth_traces(12, N, seed=3)
    first = [0, 1, 4, 4, 12]
    S = abi.OracleFrame.from_params(p, N).S
    ls, ts, ls_env, ts_env = bbr.expected(p, X, first, [(0, S), (0, S // 2 + 1), (S // 2 + 1, S), (3, 3)])
    for b in range(4):
        seg = X[first[b]:first[b + 1]]
        if not len(seg):
            assert not any(o[b].any() for o in (ls, ts, ls_env, ts_env))
            continue
        w = abi.run_main(abi.oracle().orc_tspws_main, p, seg)
        assert w["rc"] == 0
        assert np.array_equal(ls[b, 0], w["ls"]) and np.array_equal(ts[b, 0], w["tsPWS"])
        assert abi.relerr(ts[b, 1].astype(np.float64) + ts[b, 2], w["tsPWS"]) < 2e-7 and abi.relerr(ls[b, 1].astype(np.float64) + ls[b, 2], w["ls"]) < 2e-7
        assert (ts_env[b, :3] >= np.abs(ts[b, :3])).all() and (ls_env[b, :3] >= np.abs(ls[b, :3])).all()
        assert not any(o[b, 3].any() for o in (ls, ts, ls_env, ts_env))
