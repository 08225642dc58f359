"""CPU tests of the moving-window cross-spectrum call's host side and of its checker (tests/mwcs_rows_ref.py).  No GPU: the library is loaded
for its host functions only (tspws_mwcs_basis, tspws_mwcs_bins).

  the checker's stage 1 (longdouble, with its any-order bound) against an independent numpy.fft.rfft evaluation on the parity batch, for
  the three parameter sets of the GPU test; a deliberately wrong window (one sample off) is outside the bound
  tspws_mwcs_basis against longdouble: every entry of g, C and S within 1 ulp, Tc and Ts bit-equal to the ascending-l FP64 sums of the entries
  tspws_mwcs_bins against its definition, and its refusals
  the window enumeration of the binding against the definition
  a seed in 0 .. 19 whose parity batch has no term that FP64 rounding could flip, judged from a plain numpy FP64 stage 1
  recovery: a band-limited noise reference stretched by stretch_rows_ref's cubic convolution at eps = 1e-3.  The tolerance on eps_hat and
  eps0, mwcs_rows_ref.RTOL = 5 % of eps, is fixed from the checker's own output on this input (eps_hat 1.0330e-3 and 0.9910e-3, eps0
  1.0028e-3 and 0.9880e-3 on the two lag ranges: 3.3 % at the worst), no property of the library; it also pins the sign."""
import importlib

import numpy as np
import pytest

import mwcs_rows_ref as mr

tspws = importlib.import_module("ts-pws_amd")


@pytest.fixture(scope="module")
def tabs():
    return {k: tspws.mwcs_basis(p.kwargs()) for k, (p, _) in mr.SETS.items()}


@pytest.mark.parametrize("name", tuple(mr.SETS))
def test_basis_against_longdouble(tabs, name):
    par, _ = mr.SETS[name]
    tab = tabs[name]
    assert tab["C"].shape == (par.L, par.Qx) and tab["k"].shape == (2 * par.h + 1,) and tab["v"].shape == (par.Qx,)
    ideal = mr.basis(par)
    assert mr.ulps(tab["g"], ideal["g"]).max() <= 1 and (tab["g"] > 0).all() and (tab["g"] <= 1).all()
    Cs, Ss = mr.ideal_table(par, tab["g"])
    worst = max(mr.ulps(tab["C"], Cs).max(), mr.ulps(tab["S"], Ss).max())
    print(name, "worst table entry:", worst, "ulp")
    assert worst <= 1
    # exact zeros and ones of the angle are exact
    assert (tab["S"][0] == 0).all() and np.array_equal(tab["C"][0], np.full(par.Qx, tab["g"][0]))
    # Tc, Ts: the entries added in ascending l, in FP64
    for T, E in ((tab["Tc"], tab["C"]), (tab["Ts"], tab["S"])):
        acc = np.zeros(par.Qx)
        for l in range(par.L):
            acc = acc + E[l]
        assert np.array_equal(acc, T)
    assert np.array_equal(tab["v"], (2.0 * np.pi) * np.arange(par.qa, par.qb, dtype=np.float64) / np.float64(par.P))
    assert tab["k"][par.h] == 1.0 and np.array_equal(tab["k"], tab["k"][::-1]) and (tab["k"] > 0).all()
    np.testing.assert_allclose(tab["k"], 0.5 * (1 + np.cos(np.pi * np.arange(-par.h, par.h + 1) / (par.h + 1))), rtol=1e-15, atol=0)


def test_bins():
    for P, dt, lo, hi in ((512, 0.05, 0.5, 2.0), (128, 1.0, 0.02, 0.16), (4096, 0.01, 0.0, 1e9), (16, 1.0, 0.1, 0.3), (1024, 0.04, 0.1, 1.0)):
        s = np.float64(P) * np.float64(dt)
        q0 = int(min(max(1, np.ceil(np.float64(lo) * s)), P // 2))
        q1 = int(min(P // 2, np.ceil(np.float64(hi) * s)))
        assert tspws.mwcs_bins(P, dt, lo, hi) == (q0, q1), (P, dt, lo, hi)
        inside = [q for q in range(1, P // 2) if lo <= q / s < hi]
        assert inside == list(range(q0, q1))
    for bad in ((100, 1.0, 0.1, 0.3), (8192, 1.0, 0.1, 0.3), (128, 0.0, 0.1, 0.3), (128, 1.0, -0.1, 0.3), (128, 1.0, 0.3, 0.3), (128, 1.0, 0.1, float("nan")),
                (128, 1.0, 0.1, 0.105)):
        with pytest.raises(tspws.TspwsError, match="tspws_mwcs_bins refused"):
            tspws.mwcs_bins(*bad)


def test_window_enumeration():
    for name, (par, ranges) in mr.SETS.items():
        want = mr.windows(par, ranges)
        got = tspws.mwcs_windows(tspws.mwcs_par(**par.kwargs()), ranges)
        assert [tuple(r) for r in got.tolist()] == want
        assert all(n + par.L <= ranges[w][1] and n >= ranges[w][0] for n, w in want)
        # no further window fits a range
        for w, (n0, n1) in enumerate(ranges):
            mine = [n for n, ww in want if ww == w]
            assert (not mine and n1 - n0 < par.L) or (mine[0] == n0 and mine[-1] + par.hop + par.L > n1 and np.all(np.diff(mine) == par.hop))
    assert len(mr.windows(*mr.SETS["i"])) == 73 and mr.SETS["ii"][0].Qx == 64 and mr.SETS["iii"][0].qa == 0
    # the last window of the third range ends at column N - 1
    for par, ranges in mr.SETS.values():
        assert max(n for n, w in mr.windows(par, ranges) if w == 2) + par.L == mr.N


@pytest.mark.parametrize("name", tuple(mr.SETS))
def test_checker_stage1_against_rfft(tabs, name):
    par, ranges = mr.SETS[name]
    rows, ref, _ = mr.parity_batch(0)
    wins = mr.windows(par, ranges)
    x = rows[:2].reshape(-1, rows.shape[-1])
    re, im, bre, bim = mr.stage1(x, par, wins, tabs[name]["g"])
    got = mr.fp64_stage1(x, par, wins, tabs[name]["g"])
    # numpy's FFT is another FP64 algorithm with O(log P) roundings on top of the demeaning and tapering in FP64: its own error, a small
    # multiple of u (sum |x| + |mu| L), is added to the bound
    X = mr.frames(x, par, wins)
    fft_err = mr.K * (3 * np.log2(par.P) + 8) * mr.u * (np.abs(X).sum(axis=-1) + np.abs(X.mean(axis=-1)) * par.L)[..., None]
    w1 = mr.check(f"set {name} Re F against rfft", got.real, re, bre + fft_err)
    w2 = mr.check(f"set {name} Im F against rfft", got.imag, im, bim + fft_err)
    assert w1 <= 1 and w2 <= 1
    # a window taken one sample late is far outside
    late = mr.fp64_stage1(x, par, [(min(n + 1, mr.N - par.L), w) for n, w in wins], tabs[name]["g"])
    moved = np.array([min(n + 1, mr.N - par.L) != n for n, _ in wins])
    live = (np.abs(x[:, :mr.N]).max(axis=-1) > 0)
    assert (np.abs(late.real - re.astype(np.float64))[live][:, moved] > (bre + fft_err).astype(np.float64)[live][:, moved]).any(axis=-1).all()


def test_a_decided_seed_exists(tabs):
    """From a plain numpy FP64 stage 1: the first seed in 0 .. 19 whose parity batch holds no undecided term, for every parameter set."""
    for seed in range(20):
        rows, ref, mtr = mr.parity_batch(seed)
        und = [mr.reference(rows, ref, par, ranges, mr.Z, tabs[name], mtr=mtr)["undecided"] for name, (par, ranges) in mr.SETS.items()]
        print("seed", seed, "undecided terms per set:", und)
        if not any(und):
            break
    else:
        raise AssertionError("no seed in 0 .. 19 decides every term")
    # the all-zero row and the reference that is zero inside the last range give NaN windows; the rows left out NaN and n = -1
    par, ranges = mr.SETS["i"]
    want = mr.reference(rows, ref, par, ranges, mr.Z, tabs["i"], mtr=mtr)
    w3 = [j for j, (_, w) in enumerate(want["wins"]) if w == 3]
    assert np.isnan(want["win"][0, 5]).all() and np.isnan(want["win"][1][:, w3]).all() and not np.isnan(want["win"][0, 0]).any()
    assert (want["fit"][mtr == 0][..., 5] == -1).all() and (want["fit"][0, 5, :, 5] == 0).all() and (want["fit"][..., 1, 5][mtr > 0] == 0).all()


def test_recovery_and_sign():
    ref, row = mr.recovery_rows()
    tab = tspws.mwcs_basis(mr.RPAR.kwargs())
    want = mr.reference(row[None, None], ref[None], mr.RPAR, mr.RRANGES, mr.RZ, tab)
    for w in range(2):
        eh, ic, ee, e0, r0, n = want["fit"][0, 0, w]
        print(f"range {w}: eps_hat {eh:.6e} +- {ee:.2e}, icpt {ic:+.4f}, eps0 {e0:.6e} +- {r0:.2e}, n {n:.0f}")
        assert n >= 8
        assert abs(eh - mr.REPS) <= mr.RTOL * mr.REPS and abs(e0 - mr.REPS) <= mr.RTOL * mr.REPS
    # the sign: the mirrored pair (the row as reference) gives the opposite sign
    back = mr.reference(ref[None, None], row[None], mr.RPAR, mr.RRANGES, mr.RZ, tab)
    assert (back["fit"][0, 0, :, 0] < 0).all() and (want["fit"][0, 0, :, 0] > 0).all()
