"""CPU-side checks of the group-arrival calls (tspws_hip_ftan_coef, tspws_hip_ftan_rows) and their host helpers: the library exports the
entry points and the binding declares them; every refusal that needs no device, with a NULL plan, host dummies and sentinel-filled outputs
unchanged; tspws_ftan_windows and tspws_ftan_periods against their formulas, and their refusals; and the checker's own tests
(tests/ftan_rows_ref.py) on coefficient sets of the oracle's forward transform: its peaks against a brute-force loop over the indices that
follows the contract sentence by sentence, the constructed sets against the peak lists they were built for, and the recovery of the group
arrivals of Gaussian wave packets.

Recovery, measured with the oracle's sets and the contract's definition: the worst |tg + z - t0| is 0.111 D_s (s = 20), the others are at
most 0.09 D_s; the condition is 0.25 D_s."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import abi
import ftan_rows_ref as fr_

tspws = importlib.import_module("ts-pws_amd")

NAMES = ("tspws_hip_ftan_coef", "tspws_hip_ftan_rows", "tspws_hip_ftan_rows_stats", "tspws_ftan_windows", "tspws_ftan_periods")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(tspws.LIB_PATH):
        tspws.build()
    return tspws.load()


def test_entry_points(lib):
    for n in NAMES:
        assert hasattr(lib, n) and n in tspws.SYMBOLS, n
    for n in ("ftan_coef", "ftan_rows", "ftan_rows_stats"):
        assert hasattr(tspws.Plan, n), n
    assert callable(tspws.ftan_windows) and callable(tspws.ftan_periods)
    stats = (C.c_uint * 5)()
    assert lib.tspws_hip_ftan_rows_stats(None, C.byref(stats)) == -1
    assert b"ftan_rows_stats: NULL" in lib.tspws_hip_last_error()


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------
def call(lib, coef, a=True, win=(((3, 9), (0, 16)),) * 2, winp=True, noise=((1, 5),) * 2, peaks=True, noise_out=True, z=7.5, W=None, P=2, scales=(0, 2), **kw):
    """One call with a NULL plan and host dummies for the device pointers (never dereferenced: every call here is refused before device work)."""
    x = np.full(16, 7.0)
    o_peaks, o_noise = np.full(64, -3.0), np.full(64, -4.0)
    w = np.array(win, dtype=np.uint64)
    nz = None if noise is None else np.array(noise, dtype=np.uint64)
    W = w.shape[1] if W is None else W
    tail = (z, scales[0], scales[1], w.ctypes.data if winp else None, W, None if nz is None else nz.ctypes.data, P, 0, o_peaks.ctypes.data if peaks else None,
            o_noise.ctypes.data if noise_out else None, None)
    if coef:
        rc = lib.tspws_hip_ftan_coef(None, x.ctypes.data if a else None, None, kw.get("nrow", 2), kw.get("B", 2), *tail)
    else:
        rc = lib.tspws_hip_ftan_rows(None, x.ctypes.data if a else None, kw.get("ld", 256), kw.get("B", 2), kw.get("M", 3), None, *tail)
    assert (o_peaks == -3.0).all() and (o_noise == -4.0).all() and (x == 7.0).all()  # outputs untouched
    return rc, lib.tspws_hip_last_error()


@pytest.mark.parametrize("coef", (True, False))
def test_refusals_without_a_plan(lib, coef):
    who = b"ftan_coef: " if coef else b"ftan_rows: "
    # the NULL plan itself, with everything else in order (also without noise, empty, and with what only the plan can judge)
    for kw in (dict(), dict(noise=None, noise_out=False), dict(noise_out=False), dict(B=0), dict(M=0), dict(nrow=0), dict(ld=3), dict(win=(((0, 10 ** 9),),) * 2),
               dict(scales=(0, 10 ** 6)), dict(noise=((0, 10 ** 9),) * 2), dict(z=-1e300), dict(nrow=5)):
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + b"NULL" in err, (kw, err)
    for kw in (dict(a=False), dict(winp=False), dict(peaks=False)):
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + b"NULL" in err, (kw, err)
    cases = ((dict(W=0), b"1 to 4 windows"), (dict(W=5), b"1 to 4 windows"), (dict(P=0), b"1 to 4 peaks"), (dict(P=5), b"1 to 4 peaks"),
             (dict(scales=(2, 2)), b"an empty scale range (s_begin >= s_end)"), (dict(scales=(3, 1)), b"an empty scale range (s_begin >= s_end)"),
             (dict(noise=None), b"a noise output without a noise range"),
             (dict(win=(((3, 9), (0, 16)), ((3, 9), (5, 5)))), b"an empty window (n0 >= n1)"), (dict(win=(((9, 3),),) * 2), b"an empty window (n0 >= n1)"),
             (dict(noise=((1, 5), (5, 5))), b"an empty noise range (q0 >= q1)"), (dict(noise=((1, 5), (6, 5)), noise_out=False), b"an empty noise range (q0 >= q1)"),
             (dict(z=float("nan")), b"a NaN or infinite zero-lag position"), (dict(z=float("-inf")), b"a NaN or infinite zero-lag position"))
    for kw, text in cases:
        rc, err = call(lib, coef, **kw)
        assert rc == -1 and who + text in err, (kw, err)
    # more than 2^32 - 16 rows: from the counts alone, before a table is read (the tables here hold 2 ensembles)
    rc, err = call(lib, coef, nrow=0xfffffff1, B=0xfffffff1) if coef else call(lib, coef, B=0x10000, M=0x10000)
    assert rc == -1 and who + b"more than 2^32 - 16 rows" in err, err


# ---- the host helpers -----------------------------------------------------------------------------------------------------------------------
def test_windows_against_the_formula(lib):
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(300):
        dist, vmin, dt = rng.uniform(0, 400), rng.uniform(0.5, 3), rng.choice([0.05, 0.5, 1.0, 2.0])
        vmax, z, N = vmin * rng.uniform(1, 3), rng.choice([2048.0, 2048.25, 100.5, 0.0]), int(rng.choice([4096, 1501]))
        lo = [math.ceil(z + dist / (vmax * dt)), math.ceil(z - dist / (vmin * dt))]
        hi = [math.floor(z + dist / (vmin * dt)) + 1, math.floor(z - dist / (vmax * dt)) + 1]
        for sides in (1, 2):
            want = [(max(a, 0), min(b, N)) for a, b in zip(lo[:sides], hi[:sides])]
            win = np.full((2, 2), 77, np.uint64)
            rc = lib.tspws_ftan_windows(dist, vmin, vmax, dt, z, N, sides, win.ctypes.data)
            if all(a < b for a, b in want):
                assert rc == 0 and [tuple(int(v) for v in r) for r in win[:sides]] == want and (win[sides:] == 77).all(), (dist, vmin, vmax, dt, z, N, sides, win, want)
                assert np.array_equal(tspws.ftan_windows(dist, vmin, vmax, dt, z, N, sides), win[:sides])
                n += 1
            else:
                assert rc == -1 and b"ftan_windows: an empty window" in lib.tspws_hip_last_error() and (win == 77).all()
    assert n > 100
    # an exact case: 100 km at 2 .. 4 km/s, dt = 1 s, z = 2048: lags 25 .. 50 on both sides
    assert tspws.ftan_windows(100.0, 2.0, 4.0, 1.0, 2048.0, 4096, 2).tolist() == [[2073, 2099], [1998, 2024]]


def test_windows_refusals(lib):
    win = np.full((2, 2), 77, np.uint64)
    good = dict(dist=100.0, vmin=2.0, vmax=4.0, dt=1.0, z=2048.0, N=4096, sides=2)

    def run(p=win.ctypes.data, **kw):
        a = dict(good, **kw)
        rc = lib.tspws_ftan_windows(a["dist"], a["vmin"], a["vmax"], a["dt"], a["z"], a["N"], a["sides"], p)
        assert (win == 77).all()  # nothing written
        return rc, lib.tspws_hip_last_error()

    assert run(p=None) == (-1, b"ftan_windows: NULL")
    for kw in (dict(sides=0), dict(sides=3)):
        assert run(**kw) == (-1, b"ftan_windows: sides must be 1 or 2"), kw
    for kw in (dict(dist=-1.0), dict(dist=float("nan")), dict(vmin=0.0), dict(vmin=5.0), dict(vmax=float("inf")), dict(dt=0.0), dict(dt=-1.0), dict(z=float("nan"))):
        rc, err = run(**kw)
        assert rc == -1 and err.startswith(b"ftan_windows: needs finite"), (kw, err)
    for kw in (dict(z=5000.0), dict(sides=2, z=10.0), dict(N=0), dict(dist=1e6)):
        assert run(**kw) == (-1, b"ftan_windows: an empty window"), kw
    with pytest.raises(tspws.TspwsError, match="ftan_windows: an empty window"):
        tspws.ftan_windows(100.0, 2.0, 4.0, 1.0, 5000.0, 4096)


def test_periods(lib):
    scale = 2.0 * 2.0 ** (np.arange(36) / 4.0)
    for w0, dt in ((6.0, 1.0), (abi.W0_DEFAULT, 0.05), (5.336, 2.5)):
        T = np.zeros(36)
        assert lib.tspws_ftan_periods(scale.ctypes.data, 36, w0, dt, T.ctypes.data) == 0
        assert np.array_equal(T, 2 * math.pi * dt * scale / w0)     # the operations in that order
        _, fc = tspws.bands_from_frequencies((scale, w0), dt, [0.0, 1.0])
        assert np.allclose(T * fc, 1.0, rtol=4e-16, atol=0)         # the inverse of the centre frequency
        assert np.array_equal(tspws.ftan_periods((scale, w0), dt), T) and np.array_equal(tspws.ftan_periods(dict(scale=scale, w0=w0), dt), T)
    T = np.full(36, 77.0)
    for args, text in (((None, 36, 6.0, 1.0, T.ctypes.data), b"NULL"), ((scale.ctypes.data, 36, 6.0, 1.0, None), b"NULL"),
                       ((scale.ctypes.data, 36, 6.0, 0.0, T.ctypes.data), b"dt must be positive"), ((scale.ctypes.data, 36, 6.0, float("nan"), T.ctypes.data), b"dt must be positive"),
                       ((scale.ctypes.data, 36, 0.0, 1.0, T.ctypes.data), b"w0 must be positive"), ((scale.ctypes.data, 36, float("inf"), 1.0, T.ctypes.data), b"w0 must be positive")):
        assert lib.tspws_ftan_periods(*args) == -1 and lib.tspws_hip_last_error() == b"ftan_periods: " + text and (T == 77.0).all(), text
    assert lib.tspws_ftan_periods(None, 0, 6.0, 1.0, None) == 0


# ---- the checker's own tests ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    return fr_.Frame.from_oracle(abi.resolve(abi.default_params(), fr_.N), fr_.N)


def brute(fr, s, ys, win, z, skip, P):
    """The contract, sentence by sentence, one index at a time, in Python floats (IEEE double, each operation rounded on its own)."""
    D, Ns, c, L = int(fr.D[s]), int(fr.Ns[s]), int(fr.c[s]), int(fr.L[s])

    def a2(k):
        re, im = float(ys[k].real), float(ys[k].imag)
        return re * re + im * im

    found = []
    for k in range(Ns):
        if not win[0] <= k * D < win[1]:
            continue
        if skip and not (k * D - c >= 0 and k * D - c + L <= fr.N):
            continue
        if not 1 <= k <= Ns - 2:
            continue
        am, a0, ap = a2(k - 1), a2(k), a2(k + 1)
        if not (math.isfinite(am) and math.isfinite(a0) and math.isfinite(ap)):
            continue
        if a0 > am and a0 >= ap:
            found.append((-a0, k, am, ap))
    found.sort()
    out = []
    for na0, k, am, ap in found[:P]:
        a0 = -na0
        den = (am - 2.0 * a0) + ap
        d = 0.5 * (am - ap) / den if den != 0 else 0.0
        out.append([(float(k) + d) * float(D) - z, math.sqrt(a0), float(ys[k].real), float(ys[k].imag), float(k)])
    return np.array(out + [[np.nan] * 4 + [-1.0]] * (P - len(out)))


def test_checker_against_the_brute_force_loop(frame):
    rows, _ = fr_.parity_batch(0)
    npk = 0
    for b, m in ((0, 0), (1, 2), (2, 3)):
        Y = frame.oracle.forward(rows[b, m, :fr_.N].astype(np.float64))
        for z, skip, P in ((750.0, False, 4), (750.25, True, 3), (750.0, True, 1)):
            want = fr_.reference(frame, Y[None], z, fr_.PWIN[b], (0, frame.S), P, skip_wrapped=skip)["peaks"]
            for s in range(frame.S):
                ys = Y[frame.off[s]:frame.off[s + 1]]
                for w in range(2):
                    got = brute(frame, s, ys, fr_.PWIN[b, w], z, skip, P)
                    assert fr_.same(got, want[0, w, s]), (b, m, z, skip, P, s, w)
                    npk += int((got[:, 4] >= 0).sum())
    print("peaks compared:", npk)
    assert npk > 300


def test_constructed_sets(frame):
    Y, win, noise, want = fr_.constructed(frame)
    ref = fr_.reference(frame, Y, fr_.Z, win, (0, 3), 4, ens=np.zeros(len(Y), np.uint32), noise=noise)
    for i, name in enumerate(fr_.CNAMES):
        for w, ks in ((0, want[name]), (1, fr_.CWHOLE.get(name, want[name]))):
            got = ref["peaks"][i, w, fr_.CS, :, 4]
            exp = (ks + [-1] * 4)[:4]
            assert got.tolist() == exp, (name, w, got, exp)
            assert np.isnan(ref["peaks"][i, w, fr_.CS, len(ks):, :4]).all() and not np.isnan(ref["peaks"][i, w, fr_.CS, :min(len(ks), 4), :4]).any()
            ys = Y[i, frame.off[fr_.CS]:frame.off[fr_.CS + 1]]
            assert fr_.same(brute(frame, fr_.CS, ys, win[w], fr_.Z, False, 4), ref["peaks"][i, w, fr_.CS])
        assert (ref["peaks"][i, :, 1:, :, 4] == -1).all()       # the other scales hold nothing
    # den == 0 gives the index itself; the noise sums leave out exactly the two non-finite coefficients; the all-zero row sums to 0
    i = fr_.CNAMES.index("den0")
    a2 = fr_.a2_of(Y[i, frame.off[fr_.CS] + 320:frame.off[fr_.CS] + 323])
    assert a2[1] > a2[0] and (a2[0] - 2.0 * a2[1]) + a2[2] == 0 and ref["peaks"][i, 0, fr_.CS, 0, 0] == 321 * 2 - fr_.Z
    nm = fr_.members(frame, fr_.CS, noise, False).size
    assert ref["undecided"] == 0 and (ref["n"][:, 0] == [nm - 2 if n == "inf_nan" else nm for n in fr_.CNAMES]).all()
    assert ref["Q"][fr_.CNAMES.index("zero"), 0] == 0 and ref["Q"][fr_.CNAMES.index("equal"), 0] == 70


def test_recovery_input():
    """The group arrivals of the recovery row from the oracle's sets: within 0.25 D_s of the packets' centres."""
    fr = fr_.Frame.from_oracle(abi.resolve(abi.default_params(), fr_.RN), fr_.RN)
    assert fr.S == 36 and fr.D[4] == fr.D[7] and fr.D[4] != fr.D[8]  # 36 scales, 4 voices
    row, t0s = fr_.recovery_row(fr)
    Y = fr.oracle.forward(row.astype(np.float64))[None]
    peaks = fr_.reference(fr, Y, fr_.RZ, fr_.RWIN, (0, fr.S), 1)["peaks"]
    worst = fr_.check_recovery(fr, peaks[:, 0], t0s, "oracle sets")
    print(f"worst {worst:.3f} D_s")
