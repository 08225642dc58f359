"""GPU tests of the wavelet cross-spectrum calls (tspws_hip_wxs_coef, tspws_hip_wxs_rows), on the shipped library, against the checker
tests/wxs_rows_ref.py.

Parity: the batch of wxs_rows_ref.parity_batch (N = 1501, odd, no D divides it; ld = N + 3 and ldr = N + 1 with NaN pad columns; B = 3,
M = 9 with counts that leave out 0 / 4 / 8 rows; three windows whose edges are no multiples of any D, one touching both trace ends; five
bands: one octave, one cut between voices, two overlapping, one empty; noise of sigma 0, 0.2, 1; scales of 1e-6 .. 1e2; an all-zero row; a
reference that is zero inside a window) at z = 750, 0 and 750.25, with and without the wrap rule.  The coefficient sets come from
Plan.forward on the device and are downloaded; the checker runs on those bits: every sum inside its bound, n exact, NaN exactly where the
checker has NaN.  The seed is the first one whose sets hold no term whose phase FP64 rounding could flip between +pi and -pi and none whose
participation is undecided: a condition on the inputs, evaluated by the checker alone.  Then the fit bit for bit, wxs_rows against wxs_coef,
the independence properties bit for bit, three rounds under a small budget in a child process, recovery of a known stretch (which pins the
sign), the refusals that need a plan, and the outputs' hygiene.

Measured on one MI355X (profiles/wxs_rows_parity.txt): seed 0; the largest |error| / bound over the six parity calls is 0.055 (Att; every sum
between 0.023 and 0.055)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import wxs_rows_child as wxc
import wxs_rows_ref as wr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N = wr.N
B, M, W, R = 3, 9, 3, 5
NAN = float("nan")


def same(a, b):
    """Bit equality of two float64 arrays, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def lib():
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    return lib


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan(lib, torch):
    return tspws.Plan(tspws.resolve(abi.default_params(), N), N)


@pytest.fixture(scope="module")
def frame(plan):
    return wr.Frame.from_plan(plan)


@pytest.fixture(scope="module")
def bands(frame):
    return wr.parity_bands(frame)


@pytest.fixture(scope="module")
def batch(torch, plan, frame, bands):
    """The parity batch of the first seed whose device coefficient sets decide every term, at every z and with both wrap rules, with the
    checker's answers: computed once, never changed.  dict(rows, ref, mtr (host), d_rows, d_ref, Yc, Yr (device), ens, want[(z, skip)])."""
    ens = np.arange(B * M, dtype=np.uint32) // M
    for seed in range(20):
        rows, ref, mtr = wr.parity_batch(seed, B, M)
        d_rows, d_ref = torch.from_numpy(rows).cuda(), torch.from_numpy(ref).cuda()
        Yc = plan.forward(d_rows.view(B * M, N + 3)[:, :N])
        Yr = plan.forward(d_ref[:, :N])
        hc, hr = Yc.cpu().numpy(), Yr.cpu().numpy()
        assert np.isfinite(hc).all() and np.isfinite(hr).all()
        want = {(z, skip): wr.reference(frame, hc, hr, z, bands, wr.WINDOWS, ens=ens, skip_wrapped=skip) for z in wr.ZS for skip in (False, True)}
        if all(w["flips"] == 0 and w["undecided"] == 0 for w in want.values()):
            print("parity batch: seed", seed)
            return dict(seed=seed, rows=rows, ref=ref, mtr=mtr, d_rows=d_rows, d_ref=d_ref, Yc=Yc, Yr=Yr, ens=ens, want=want)
    raise AssertionError("no seed in 0 .. 19 decides every term")


@pytest.fixture(scope="module")
def full(plan, batch, bands):
    """(sums, fit) of wxs_rows on the parity batch at z = 750 without the wrap rule, as numpy: what the independence tests compare against."""
    sums, fit = plan.wxs_rows(batch["d_rows"][:, :, :N], batch["d_ref"][:, :N], wr.Z, bands, wr.WINDOWS, mtr=batch["mtr"], sums=True)
    return sums.cpu().numpy(), fit.cpu().numpy()


def expected_stats(frame, bands, windows, skip, rows, left_out, rounds=1):
    """The stats from the definition: the scales inside a band, and per (scale, window) the members in segments of 256."""
    used = sorted({s for a, b in bands for s in range(a, b)})
    items = sum(-(-wr.members(frame, s, w, skip).size // 256) for s in used for w in windows)
    return dict(rounds=rounds, rows=rows, left_out=left_out, items=items, scales=len(used))


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("z", wr.ZS)
def test_parity_and_fit(plan, frame, bands, batch, z, skip):
    rows, ref = batch["rows"], batch["ref"]
    assert np.isnan(rows[:, :, N:]).all() and np.isnan(ref[:, N:]).all() and np.isfinite(rows[:, :, :N]).all() and np.isfinite(ref[:, :N]).all()
    sums, fit = plan.wxs_coef(batch["Yc"], batch["Yr"], z, bands, wr.WINDOWS, ens=batch["ens"], skip_wrapped=skip, sums=True)
    sums, fit = sums.cpu().numpy(), fit.cpu().numpy()
    assert sums.shape == (B * M, W, R, 9) and fit.shape == (B * M, W, R, 6)
    st = plan.wxs_rows_stats()
    assert st == expected_stats(frame, bands, wr.WINDOWS, skip, B * M, 0), st
    worst = wr.check(sums, batch["want"][(z, skip)], f"seed {batch['seed']} z = {z} skip_wrapped = {skip}")
    assert (worst <= 1).all()
    # the segments of the finest scales are exercised: more than one item per (scale, window) somewhere
    assert st["items"] > st["scales"] * W or skip
    assert (sums[5] == 0).all() and (sums[:, :, 4] == 0).all()  # the all-zero row, the empty band: no term
    assert np.isnan(fit[5][..., :5]).all() and (fit[5][..., 5] == 0).all()
    assert not np.isnan(fit[0, 2, :4, :4]).any()                # a live row, the whole-trace window, the bands that hold scales
    # the fit: the contract's formula in numpy float64 on the library's own sums, bit for bit
    assert same(fit, wr.fit(sums))


def test_rows_equal_coef(plan, frame, bands, batch):
    mtr = batch["mtr"]
    for z, skip in ((750.0, False), (750.25, True)):
        sums, fit = plan.wxs_rows(batch["d_rows"][:, :, :N], batch["d_ref"][:, :N], z, bands, wr.WINDOWS, mtr=mtr, skip_wrapped=skip, sums=True)
        st = plan.wxs_rows_stats()
        assert st == expected_stats(frame, bands, wr.WINDOWS, skip, 9 + 5 + 1, 12), st
        sums, fit = sums.cpu().numpy(), fit.cpu().numpy()
        assert sums.shape == (B, M, W, R, 9) and fit.shape == (B, M, W, R, 6)
        c_sums, c_fit = plan.wxs_coef(plan.forward(batch["d_rows"].view(B * M, N + 3)[:, :N]), plan.forward(batch["d_ref"][:, :N]), z, bands, wr.WINDOWS,
                                      ens=batch["ens"], skip_wrapped=skip, sums=True)
        c_sums, c_fit = c_sums.cpu().numpy().reshape(sums.shape), c_fit.cpu().numpy().reshape(fit.shape)
        take = mtr > 0
        assert take.sum() == 15
        assert same(sums[take], c_sums[take]) and same(fit[take], c_fit[take])
        assert np.isnan(sums[~take]).all() and np.isnan(fit[~take][..., :5]).all() and (fit[~take][..., 5] == -1).all()
        # without h_ens: row i against set i
        one = plan.wxs_coef(batch["Yc"][9:12], batch["Yc"][:3], z, bands, wr.WINDOWS, skip_wrapped=skip).cpu().numpy()
        two = plan.wxs_coef(batch["Yc"][9:12], batch["Yc"][:3], z, bands, wr.WINDOWS, ens=np.arange(3, dtype=np.uint32), skip_wrapped=skip).cpu().numpy()
        assert same(one, two)


def test_independence(torch, plan, bands, batch, full):
    mtr = batch["mtr"]
    d_rows, d_ref = batch["d_rows"][:, :, :N], batch["d_ref"][:, :N]
    sums0, fit0 = full

    def run(r, f, bd=bands, wins=wr.WINDOWS, m=None, sums=True):
        got = plan.wxs_rows(r, f, wr.Z, bd, wins, mtr=m, sums=sums)
        return (got[0].cpu().numpy(), got[1].cpu().numpy()) if sums else got.cpu().numpy()

    # a repeated call
    s, f = run(d_rows, d_ref, m=mtr)
    assert same(s, sums0) and same(f, fit0)
    # the batch against a loop of one-ensemble calls
    for b in range(B):
        s, f = run(d_rows[b:b + 1], d_ref[b:b + 1], m=mtr[b:b + 1])
        assert same(s[0], sums0[b]) and same(f[0], fit0[b]), b
    # a row of the M = 9 call against the M = 1 call on that row
    for b, m in ((0, 0), (0, 8), (1, 2), (2, 6)):
        s, f = run(d_rows[b:b + 1, m:m + 1], d_ref[b:b + 1])
        assert same(s[0, 0], sums0[b, m]) and same(f[0, 0], fit0[b, m]), (b, m)
    # each band alone against its slot of the full table; each window alone
    for r, bd in enumerate(bands):
        s, f = run(d_rows, d_ref, bd=[bd], m=mtr)
        assert same(s[..., 0, :], sums0[..., r, :]) and same(f[..., 0, :], fit0[..., r, :]), r
    for w, win in enumerate(wr.WINDOWS):
        s, f = run(d_rows, d_ref, wins=(win,), m=mtr)
        assert same(s[:, :, 0], sums0[:, :, w]) and same(f[:, :, 0], fit0[:, :, w]), w
    # the bands in another order, with a stranger among them
    s, f = run(d_rows, d_ref, bd=[bands[3], (0, plan.S), bands[0]], m=mtr)
    assert same(s[..., 0, :], sums0[..., 3, :]) and same(s[..., 2, :], sums0[..., 0, :]) and same(f[..., 2, :], fit0[..., 0, :])
    # without the sums output
    assert same(run(d_rows, d_ref, m=mtr, sums=False), fit0)
    # the view of the padded base against a contiguous copy
    s, f = run(d_rows.contiguous(), d_ref.contiguous(), m=mtr)
    assert same(s, sums0) and same(f, fit0)


def test_small_budget_takes_rounds_bit_identically(torch, tmp_path):
    """The rounds batch under TSPWS_PART_MB=16 in a child process (3 rounds) against the one-round outputs of this process, bit for bit."""
    sums, fit, st = wxc.run(torch)
    assert st["rounds"] == 1 and st["rows"] == wxc.RB * wxc.RM - 3 and st["left_out"] == 3, st
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "wxs_rows_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "WXS_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2, int(small["rounds"])
    assert same(small["sums"], sums) and same(small["fit"], fit)
    assert not np.isnan(sums[2]).any() and np.isnan(sums[5, ::4]).all() and not np.isnan(sums[5, 1]).any()


def test_recovery(torch):
    """A row ref(t (1 + 2e-3)) gives eps_hat = +2e-3 within 10 % at coh > 0.9 (the CPU test holds the checker's own value to that), and the
    library's sums lie inside the checker's bounds."""
    pl = tspws.Plan(tspws.resolve(abi.default_params(), wr.RN), wr.RN)
    fr = wr.Frame.from_plan(pl)
    band = wr.recovery_band(fr)
    ref, row = wr.recovery_rows()
    d_row, d_ref = torch.from_numpy(row[None, None]).cuda(), torch.from_numpy(ref[None]).cuda()
    Yc, Yr = pl.forward(d_row[0]), pl.forward(d_ref)
    for skip in (False, True):
        want = wr.reference(fr, Yc.cpu().numpy(), Yr.cpu().numpy(), wr.RZ, band, wr.RWIN, skip_wrapped=skip)
        sums, fit = pl.wxs_rows(d_row, d_ref, wr.RZ, band, wr.RWIN, skip_wrapped=skip, sums=True)
        sums, fit = sums.cpu().numpy(), fit.cpu().numpy()
        f = fit[0, 0, 0, 0]
        print(f"skip_wrapped = {skip}: eps_hat {f[0]:.6e}, icpt {f[1]:+.4f}, err {f[2]:.3g}, rms {f[3]:.3g}, coh {f[4]:.4f}, n {f[5]:.0f}")
        wr.check(sums[0], want, f"recovery skip_wrapped = {skip}")
        assert same(fit, wr.fit(sums))
        assert abs(f[0] - wr.REPS) <= 0.1 * wr.REPS and f[4] > 0.9


def test_refusals_and_hygiene(torch, lib, plan, bands, batch, full):
    d_rows, d_ref, mtr = batch["d_rows"], batch["d_ref"], batch["mtr"]
    S = plan.S
    o_sums = torch.full((B * M * W * R * 9 + 64,), NAN, dtype=torch.float64, device="cuda")
    o_fit = torch.full((B * M * W * R * 6 + 64,), NAN, dtype=torch.float64, device="cuda")
    got = plan.wxs_rows(d_rows[:, :, :N], d_ref[:, :N], wr.Z, bands, wr.WINDOWS, mtr=mtr, sums=True, out=(o_sums, o_fit))
    assert got[0] is o_sums and got[1] is o_fit
    h_sums, h_fit = o_sums.cpu().numpy(), o_fit.cpu().numpy()
    assert np.isnan(h_sums[-64:]).all() and np.isnan(h_fit[-64:]).all()  # nothing past [B][M][W][R][9] / [6]
    assert same(h_sums[:-64].reshape(full[0].shape), full[0]) and same(h_fit[:-64].reshape(full[1].shape), full[1])
    # the inputs are unchanged (NaN pads included)
    assert np.array_equal(d_rows.cpu().numpy(), batch["rows"], equal_nan=True) and np.array_equal(d_ref.cpu().numpy(), batch["ref"], equal_nan=True)
    # empty inputs do nothing
    assert tuple(plan.wxs_rows(d_rows[:0, :, :N], d_ref[:0, :N], wr.Z, bands, wr.WINDOWS).shape) == (0, M, W, R, 6)

    # what only the plan can judge, through the C entry points on sentinel-filled outputs
    s_sums = torch.full((B * M * W * R * 9,), -3.0, dtype=torch.float64, device="cuda")
    s_fit = torch.full((B * M * W * R * 6,), -4.0, dtype=torch.float64, device="cuda")
    bt, wa = tspws.band_table(bands), np.ascontiguousarray(np.array(wr.WINDOWS, dtype=np.uint64))

    def rows_call(ld=N + 3, ldr=N + 1, bt=bt, wa=wa, nb=B, m=M):
        rc = lib.tspws_hip_wxs_rows(plan.h, d_rows.data_ptr(), ld, nb, m, None, d_ref.data_ptr(), ldr, wr.Z, bt.ctypes.data, bt.shape[0], wa.ctypes.data,
                                    wa.shape[0], 0, s_sums.data_ptr(), s_fit.data_ptr(), None)
        torch.cuda.synchronize()
        assert bool((s_sums == -3.0).all()) and bool((s_fit == -4.0).all())  # outputs untouched
        return rc, lib.tspws_hip_last_error()

    def coef_call(ens=None, nrow=B * M, nb=B, bt=bt, wa=wa):
        e = None if ens is None else np.ascontiguousarray(ens, dtype=np.uint32)
        rc = lib.tspws_hip_wxs_coef(plan.h, batch["Yc"].data_ptr(), batch["Yr"].data_ptr(), None if e is None else e.ctypes.data, nrow, nb, wr.Z, bt.ctypes.data,
                                    bt.shape[0], wa.ctypes.data, wa.shape[0], 0, s_sums.data_ptr(), s_fit.data_ptr(), None)
        torch.cuda.synchronize()
        assert bool((s_sums == -3.0).all()) and bool((s_fit == -4.0).all())
        return rc, lib.tspws_hip_last_error()

    far = np.array([[0, S + 1]], np.uint32)
    past = np.array([[0, N + 1]], np.uint64)
    assert rows_call(ld=N - 1) == (-1, b"wxs_rows: row stride below the trace length")
    assert rows_call(ldr=N - 1) == (-1, b"wxs_rows: reference row stride below the trace length")
    assert rows_call(bt=far) == (-1, b"wxs_rows: a band ends behind the last scale")
    assert rows_call(wa=past) == (-1, b"wxs_rows: a window past the trace length")
    assert coef_call(ens=batch["ens"], bt=far) == (-1, b"wxs_coef: a band ends behind the last scale")
    assert coef_call(ens=batch["ens"], wa=past) == (-1, b"wxs_coef: a window past the trace length")
    bad = batch["ens"].copy()
    bad[-1] = B
    assert coef_call(ens=bad) == (-1, b"wxs_coef: an ensemble index >= B")
    assert coef_call(ens=None) == (-1, b"wxs_coef: without h_ens the rows must number B")
    # more than 2^32 - 16 rows: refused from the counts alone, before any row is looked at
    assert rows_call(nb=0x10000, m=0x10000) == (-1, b"wxs_rows: more than 2^32 - 16 rows")
    assert coef_call(ens=None, nrow=0xfffffff1, nb=0xfffffff1) == (-1, b"wxs_coef: more than 2^32 - 16 rows")
    # B == 0, M == 0, nrow == 0: nothing happens
    assert rows_call(nb=0)[0] == 0 and rows_call(m=0)[0] == 0 and coef_call(ens=batch["ens"], nrow=0)[0] == 0 and coef_call(ens=batch["ens"], nb=0)[0] == 0
    with pytest.raises(tspws.TspwsError, match="wxs_rows: a window past the trace length"):
        plan.wxs_rows(d_rows[:, :, :N], d_ref[:, :N], wr.Z, bands, ((0, N + 1),))
    with pytest.raises(tspws.TspwsError, match="wxs_coef: 1 to 64 bands"):
        plan.wxs_coef(batch["Yc"], batch["Yr"], wr.Z, [(0, 1)] * 65, wr.WINDOWS, ens=batch["ens"])
