"""GPU tests of tspws_hip_mwcs_rows, on the shipped library, against the checker tests/mwcs_rows_ref.py.

Parity: the batch of wxs_rows_ref.parity_batch (N = 1501 and the shipped default plan; ld = N + 3 and ldr = N + 1 with NaN pad columns;
B = 3, M = 9 with counts that leave out 0 / 4 / 8 rows; noise of sigma 0, 0.2, 1; scales of 1e-6 .. 1e2; an all-zero row; a reference that
is zero inside one lag range) under the three parameter sets of mwcs_rows_ref.SETS -- (i) L = 100, hop 37, P = 128, bins [3, 20), h = 2:
L no multiple of 4, J = 73; (ii) L = hop = P = 1024, bins [20, 68), h = 8: Qx = 64; (iii) L = P = 16, hop 1, bins [1, 3), h = 2: qa clips at
0, J = 2565 -- with four lag ranges each (one touching both trace ends, one shorter than L, one whose last window ends at column N - 1, one
overlapping another) at z = 750, 0 and 750.25.  Stage 1 (spec=True) inside the checker's any-order bound at every bin, for rows and
references; d_win inside its bound from the device's stage-1 bits; d_fit bit-equal to the formula evaluated in numpy from the device's
d_win; NaN exactly where the checker has NaN; n exact.  The seed is the first one in 0 .. 19 for which the checker, on the device's stage-1
bits, counts no term whose outcome FP64 rounding could flip: a condition on the inputs, judged by the checker alone.  Then the
independence properties bit for bit, three rounds under a small budget in a child process, the stats, the outputs' hygiene, and recovery of
a known stretch in the sign of stretch_rows.

Measured on one MI355X (profiles/mwcs_rows_parity.txt): seed 0; the largest |error| / bound is 0.18 in stage 1 (set (iii)) and 0.13 in
stage 2 (mcoh, set (iii))."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import mwcs_rows_child as mwc
import mwcs_rows_ref as mr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N = mr.N
B, M, W = 3, 9, 4
NAN = float("nan")


def same(a, b):
    """Bit equality of two float64 / complex128 arrays, NaN matching NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    a, b = a.view(np.float64), b.view(np.float64)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


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
def tabs():
    return {k: tspws.mwcs_basis(p.kwargs()) for k, (p, _) in mr.SETS.items()}


def call(plan, d_rows, d_ref, name, z=mr.Z, mtr=None, ranges=None, win=True, spec=True):
    par, rg = mr.SETS[name]
    out = plan.mwcs_rows(d_rows, d_ref, z, par.kwargs(), rg if ranges is None else ranges, mtr=mtr, win=win, spec=spec)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()} if isinstance(out, dict) else out.cpu().numpy()


@pytest.fixture(scope="module")
def batch(torch, plan, tabs):
    """The parity batch of the first seed whose device spectra decide every term under every parameter set, with the device's outputs at
    z = 750 and the checker's stage 2 on those bits: computed once, never changed."""
    for seed in range(20):
        rows, ref, mtr = mr.parity_batch(seed, B, M)
        d_rows, d_ref = torch.from_numpy(rows).cuda(), torch.from_numpy(ref).cuda()
        take = mtr > 0
        got, s2, und = {}, {}, 0
        for name, (par, ranges) in mr.SETS.items():
            got[name] = call(plan, d_rows[:, :, :N], d_ref[:, :N], name, mtr=mtr)
            spec, sref = got[name]["spec"], got[name]["spec_ref"]
            assert np.isfinite(sref.view(np.float64)).all() and np.isfinite(spec[take].view(np.float64)).all()
            s2[name] = mr.stage2(spec[take], np.broadcast_to(sref[:, None], spec.shape)[take], par, tabs[name])
            und += s2[name]["undecided"] + mr.takes_part(s2[name], par)[1]
        if und == 0:
            print("parity batch: seed", seed)
            return dict(seed=seed, rows=rows, ref=ref, mtr=mtr, take=take, d_rows=d_rows, d_ref=d_ref, got=got, s2=s2)
    raise AssertionError("no seed in 0 .. 19 decides every term")


@pytest.mark.parametrize("name", tuple(mr.SETS))
def test_parity(plan, tabs, batch, name):
    par, ranges = mr.SETS[name]
    rows, ref, mtr, take = batch["rows"], batch["ref"], batch["mtr"], batch["take"]
    assert np.isnan(rows[:, :, N:]).all() and np.isnan(ref[:, N:]).all() and np.isfinite(rows[:, :, :N]).all() and np.isfinite(ref[:, :N]).all()
    wins = mr.windows(par, ranges)
    J = len(wins)
    got = batch["got"][name]
    assert got["fit"].shape == (B, M, W, 6) and got["win"].shape == (B, M, J, 3) and got["spec"].shape == (B, M, J, par.Qx) and got["spec_ref"].shape == (B, J, par.Qx)
    # stage 1, rows and references, at every bin of [qa, qb)
    worst = {}
    for what, x, spec in (("rows", rows[take], got["spec"][take]), ("references", ref, got["spec_ref"])):
        re, im, bre, bim = mr.stage1(x, par, wins, tabs[name]["g"])
        worst["stage 1 " + what] = max(mr.check(f"set ({name}) stage 1 Re, {what}", spec.real, re, bre), mr.check(f"set ({name}) stage 1 Im, {what}", spec.imag, im, bim))
    assert np.isnan(got["spec"][~take].view(np.float64)).all() and np.isnan(got["win"][~take]).all()
    assert (got["spec"][0, 5] == 0).all()  # the all-zero row: exact zeros
    # stage 2 from the device's stage-1 bits
    s2 = batch["s2"][name]
    for i, k in enumerate(("delta", "err", "mcoh")):
        worst["stage 2 " + k] = mr.check(f"set ({name}) stage 2 {k}", got["win"][take][..., i], s2[k], s2["b_" + k])
    nanwin = np.isnan(got["win"][..., 0])
    assert nanwin[0, 5].all()                                       # the all-zero row
    if name != "ii":
        w3 = [j for j, (_, w) in enumerate(wins) if w == 3]
        assert len(w3) > 0 and nanwin[1][:, w3].all()               # the reference that is zero inside [3, 611)
    assert not nanwin[0, 0].any() and not nanwin[2, 6].any()
    # stage 3 at every z: bit-equal to the formula on the device's own d_win; the windows, spectra and d_win do not depend on z
    take_w, _ = mr.takes_part(s2, par)
    n_want = np.stack([take_w[:, [j for j, (_, w) in enumerate(wins) if w == r]].sum(axis=-1) for r in range(W)], axis=-1)
    for z in mr.ZS:
        g = got if z == mr.Z else call(plan, batch["d_rows"][:, :, :N], batch["d_ref"][:, :N], name, z=z, mtr=mtr)
        assert same(g["win"], got["win"]) and same(g["spec"], got["spec"]) and same(g["spec_ref"], got["spec_ref"])
        assert same(g["fit"], mr.fit_rows(g["win"], par, wins, W, z, take)), z
        assert np.array_equal(g["fit"][take][..., 5], n_want) and (g["fit"][~take][..., 5] == -1).all() and np.isnan(g["fit"][~take][..., :5]).all()
        assert (g["fit"][..., 1, 5][take] == 0).all() and np.isnan(g["fit"][..., 1, :5]).all()   # the range shorter than L: no window
    st = plan.mwcs_rows_stats()
    assert st == dict(rounds=1, rows=9 + 5 + 1, left_out=12, windows=J, bins=par.Qx), st
    assert n_want.max() >= 2 or name == "ii"
    print(f"PARITY set ({name}) seed {batch['seed']} J {J} Qx {par.Qx}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_independence(torch, plan, batch):
    name = "i"
    par, ranges = mr.SETS[name]
    mtr, take = batch["mtr"], batch["take"]
    d_rows, d_ref = batch["d_rows"][:, :, :N], batch["d_ref"][:, :N]
    full = batch["got"][name]
    wins = mr.windows(par, ranges)
    keys = ("fit", "win", "spec", "spec_ref")
    # a repeated call
    again = call(plan, d_rows, d_ref, name, mtr=mtr)
    assert all(same(again[k], full[k]) for k in keys)
    # the batch against one-ensemble calls
    for b in range(B):
        one = call(plan, d_rows[b:b + 1], d_ref[b:b + 1], name, mtr=mtr[b:b + 1])
        assert all(same(one[k][0], full[k][b]) for k in keys), b
    # a row of the M = 9 call against its M = 1 call
    for b, m in ((0, 0), (0, 8), (1, 2), (2, 6)):
        one = call(plan, d_rows[b:b + 1, m:m + 1], d_ref[b:b + 1], name)
        assert all(same(one[k][0, 0], full[k][b, m]) for k in keys[:3]) and same(one["spec_ref"][0], full["spec_ref"][b]), (b, m)
    # each range alone
    for w, rg in enumerate(ranges):
        js = [j for j, (_, ww) in enumerate(wins) if ww == w]
        if not js:
            with pytest.raises(tspws.TspwsError, match="mwcs_rows: no lag range holds a window"):
                call(plan, d_rows, d_ref, name, mtr=mtr, ranges=(rg,))
            continue
        one = call(plan, d_rows, d_ref, name, mtr=mtr, ranges=(rg,))
        assert same(one["fit"][:, :, 0], full["fit"][:, :, w]) and same(one["win"], full["win"][:, :, js]) and same(one["spec"], full["spec"][:, :, js]), w
        assert same(one["spec_ref"], full["spec_ref"][:, js])
    # the reference passed as a row
    asrow = call(plan, d_ref[:, None, :], d_ref, name)
    assert same(asrow["spec"][:, 0], asrow["spec_ref"]) and same(asrow["spec_ref"], full["spec_ref"])
    # without the optional outputs
    assert same(call(plan, d_rows, d_ref, name, mtr=mtr, win=False, spec=False), full["fit"])
    assert same(call(plan, d_rows, d_ref, name, mtr=mtr, win=True, spec=False)["fit"], full["fit"])
    # the view of the padded base against a contiguous copy
    copy = call(plan, d_rows.contiguous(), d_ref.contiguous(), name, mtr=mtr)
    assert all(same(copy[k], full[k]) for k in keys)
    # every row taking part: the rows that did before keep their bits
    allin = call(plan, d_rows, d_ref, name)
    assert all(same(allin[k][take], full[k][take]) for k in keys[:3])


def test_small_budget_takes_rounds_bit_identically(torch, tmp_path):
    """The rounds batch under TSPWS_PART_MB=16 in a child process (3 rounds) against the one-round outputs of this process, bit for bit."""
    fit, win, st = mwc.run(torch)
    par, ranges = mr.SETS["iii"]
    assert st == dict(rounds=1, rows=mwc.RB * mwc.RM - 3, left_out=3, windows=len(mr.windows(par, ranges)), bins=par.Qx), st
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "mwcs_rows_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "MWCS_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2, int(small["rounds"])
    assert same(small["fit"], fit) and same(small["win"], win)
    assert not np.isnan(win[2]).all() and np.isnan(win[5, ::4]).all() and not np.isnan(win[5, 1]).all() and (fit[5, ::4, :, 5] == -1).all()


def test_hygiene(torch, lib, plan, batch):
    """Through the C entry point on outputs with 64 spare values behind each: nothing past [B][M][W][6], [B][M][J][3], [B][M][J][Qx],
    [B][J][Qx] is written, the inputs are unchanged, empty inputs do nothing."""
    import ctypes as C
    name = "i"
    par, ranges = mr.SETS[name]
    full = batch["got"][name]
    J, Qx = full["win"].shape[2], par.Qx
    sizes = dict(win=B * M * J * 3, fit=B * M * W * 6, spec=B * M * J * Qx * 2, spec_ref=B * J * Qx * 2)
    o = {k: torch.full((n + 64,), -5.0, dtype=torch.float64, device="cuda") for k, n in sizes.items()}
    cp = tspws.mwcs_par(**par.kwargs())
    wa = np.ascontiguousarray(np.array(ranges, dtype=np.uint64))
    mtr = batch["mtr"]
    rc = lib.tspws_hip_mwcs_rows(plan.h, batch["d_rows"].data_ptr(), N + 3, B, M, mtr.ctypes.data, batch["d_ref"].data_ptr(), N + 1, mr.Z, C.addressof(cp),
                                 wa.ctypes.data, W, o["win"].data_ptr(), o["fit"].data_ptr(), o["spec"].data_ptr(), o["spec_ref"].data_ptr(), None)
    assert rc == 0, lib.tspws_hip_last_error()
    for k, n in sizes.items():
        h = o[k].cpu().numpy()
        assert (h[n:] == -5.0).all(), k
        assert same(h[:n], np.ascontiguousarray(full[k]).view(np.float64).reshape(-1)), k
    assert np.array_equal(batch["d_rows"].cpu().numpy(), batch["rows"], equal_nan=True) and np.array_equal(batch["d_ref"].cpu().numpy(), batch["ref"], equal_nan=True)
    assert tuple(plan.mwcs_rows(batch["d_rows"][:0, :, :N], batch["d_ref"][:0, :N], mr.Z, par.kwargs(), ranges).shape) == (0, M, W, 6)


def test_recovery_and_sign(torch):
    """The CPU test's recovery input: eps_hat and eps0 within mwcs_rows_ref.RTOL of eps = +1e-3 on both lag ranges, and the sign of
    Plan.stretch_rows on the same rows."""
    pl = tspws.Plan(tspws.resolve(abi.default_params(), mr.RN), mr.RN)
    ref, row = mr.recovery_rows()
    d_row, d_ref = torch.from_numpy(row[None, None]).cuda(), torch.from_numpy(ref[None]).cuda()
    fit = pl.mwcs_rows(d_row, d_ref, mr.RZ, mr.RPAR.kwargs(), mr.RRANGES).cpu().numpy()
    sfit = pl.stretch_rows(d_row, d_ref, mr.RZ, tspws.stretch_grid(0.01, 201), mr.RRANGES).cpu().numpy()
    for w in range(2):
        eh, ic, ee, e0, r0, n = fit[0, 0, w]
        print(f"range {w}: eps_hat {eh:.6e} +- {ee:.2e}, icpt {ic:+.4f}, eps0 {e0:.6e} +- {r0:.2e}, n {n:.0f}; stretch_rows {sfit[0, 0, w, 0]:.6e}")
        assert n >= 8
        assert abs(eh - mr.REPS) <= mr.RTOL * mr.REPS and abs(e0 - mr.REPS) <= mr.RTOL * mr.REPS
        assert np.sign(eh) == np.sign(sfit[0, 0, w, 0]) == 1.0
