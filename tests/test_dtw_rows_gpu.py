"""GPU tests of tspws_hip_dtw_rows, on the shipped library, against the checker tests/dtw_rows_ref.py -- bit for bit: dynamic time warping
is min-plus over individually rounded FP64 operations, so the device and numpy have one answer, the integer lag path included.

Parity: the batch of wxs_rows_ref.parity_batch (N = 1501 and the shipped default plan; ld = N + 3 and ldr = N + 1 with NaN pad columns;
B = 3, M = 9 with counts that leave out 0 / 4 / 8 rows; scales of 1e-6 .. 1e2; an all-zero row; a reference that is zero inside one lag
range) at the first seed in 0 .. 19 that dtw_rows_ref.well_posed accepts (the checker alone judges; the seed is printed), under the
parameter sets of dtw_rows_ref.SETS -- (i) Lmax = 5, b = 1; (ii) Lmax = 31 and 32, b = 3: nl = 63 / 65, the lane-count edge; (iii)
Lmax = 127, b = 8 -- with the four ranges of dtw_rows_ref.RANGES (one touching both trace ends, one of length 1, one shorter than b, one
overlapping the first and holding the reference's zeros) at z = 750, 0 and 750.25.  Required: lag equal to the checker's element for
element; dist bit-equal; fit bit-equal to the formula evaluated from the device's own lag and to the checker's; NaN, -1 and INT_MIN exactly
where the contract says; ties taken by the checker inside the zero-reference range.  Then the independence properties bit for bit, three
rounds under a small budget in a child process, the stats, the outputs' hygiene, and recovery of a known stretch in the sign of
stretch_rows."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import dtw_rows_child as dc
import dtw_rows_ref as dr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N = dr.N
B, M, W = 3, 9, 4
T = sum(n1 - n0 for n0, n1 in dr.RANGES)


def same(a, b):
    """Bit equality of two float64 arrays, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
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


def call(plan, d_rows, d_ref, name, z=dr.Z, mtr=None, ranges=dr.RANGES, lag=True):
    Lmax, b = dr.SETS[name]
    out = plan.dtw_rows(d_rows, d_ref, z, dict(Lmax=Lmax, b=b), ranges, mtr=mtr, lag=lag)
    return {k: v.cpu().numpy() for k, v in out.items()} if lag else out.cpu().numpy()


@pytest.fixture(scope="module")
def batch(torch):
    """The parity batch of the first well-posed seed, on the host and on the device: computed once, never changed."""
    for seed in range(20):
        if dr.well_posed(seed, B, M):
            print("parity batch: seed", seed)
            rows, ref, mtr = dr.parity_batch(seed, B, M)
            return dict(seed=seed, rows=rows, ref=ref, mtr=mtr, take=mtr > 0, d_rows=torch.from_numpy(rows).cuda(), d_ref=torch.from_numpy(ref).cuda())
    raise AssertionError("no seed in 0 .. 19 is well-posed")


@pytest.fixture(scope="module")
def want(batch):
    """name -> the checker's (fit at z = 750, lag, ties, dead), computed when first asked for and shared."""
    memo = {}

    def get(name):
        if name not in memo:
            Lmax, b = dr.SETS[name]
            memo[name] = dr.dtw_batch(batch["rows"][:, :, :N], batch["ref"][:, :N], batch["mtr"], dr.RANGES, Lmax, b, dr.Z)
        return memo[name]
    return get


@pytest.fixture(scope="module")
def got(plan, batch):
    """name -> the device's outputs on the parity batch at z = 750, computed when first asked for and shared."""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = call(plan, batch["d_rows"][:, :, :N], batch["d_ref"][:, :N], name, mtr=batch["mtr"])
        return memo[name]
    return get


@pytest.mark.parametrize("name", tuple(dr.SETS))
def test_parity(plan, batch, want, got, name):
    Lmax, b = dr.SETS[name]
    rows, ref, mtr, take = batch["rows"], batch["ref"], batch["mtr"], batch["take"]
    assert np.isnan(rows[:, :, N:]).all() and np.isnan(ref[:, N:]).all() and np.isfinite(rows[:, :, :N]).all() and np.isfinite(ref[:, :N]).all()
    wfit, wlag, ties, dead = want(name)
    g = got(name)
    assert g["fit"].shape == (B, M, W, 6) and g["lag"].shape == (B, M, T) and g["lag"].dtype == np.int32
    assert plan.dtw_rows_stats() == dict(rounds=1, rows=9 + 5 + 1, left_out=12, lags=2 * Lmax + 1, samples=T)
    # the checker took ties inside the zero-reference range, on every participating row of ensemble 1; the all-zero row is dead, nothing else
    assert (ties[1][take[1]][:, 3] > 0).all() and dead[0, 5].all() and dead[take].sum() == W
    # the lag paths, element for element; INT_MIN exactly where the row is left out or dead
    nlag = int((g["lag"] != wlag).sum())
    print(f"PARITY set ({name}) seed {batch['seed']}: {nlag} of {wlag.size} lags differ; ties per row in the zero-reference range {ties[1][take[1]][:, 3].tolist()}")
    assert nlag == 0
    off = 0
    for w, (n0, n1) in enumerate(dr.RANGES):
        isdead = (g["lag"][:, :, off:off + n1 - n0] == dr.INT_MIN)
        assert (isdead.all(axis=-1) == dead[:, :, w]).all() and (isdead.any(axis=-1) == dead[:, :, w]).all()
        off += n1 - n0
    assert (np.abs(g["lag"][g["lag"] != dr.INT_MIN]) <= Lmax).all()
    # dist, bit for bit; the fit from the device's own lags and the checker's fit, bit for bit, at every z
    assert same(g["fit"][..., 4], wfit[..., 4])
    assert np.isnan(g["fit"][dead][:, :5]).all() and (g["fit"][dead][:, 5] == -1).all() and (g["fit"][~dead][:, 5] >= 0).all()
    alive1 = ~dead[:, :, 1]
    assert np.isnan(g["fit"][:, :, 1, :3][alive1]).all() and (g["fit"][:, :, 1, 3][alive1] == 0).all()      # n_w = 1: NaN, NaN, NaN, rms 0, dist, clip
    assert np.isfinite(g["fit"][:, :, (0, 2, 3)][~dead[:, :, (0, 2, 3)]]).all()
    for z in dr.ZS:
        gz = g if z == dr.Z else call(plan, batch["d_rows"][:, :, :N], batch["d_ref"][:, :N], name, z=z, mtr=mtr)
        assert np.array_equal(gz["lag"], g["lag"])
        assert same(gz["fit"], dr.refit(gz["lag"], gz["fit"], dr.RANGES, Lmax, z)), z
        assert same(gz["fit"], dr.refit(wlag, wfit, dr.RANGES, Lmax, z)), z
    assert same(g["fit"], wfit)


def test_independence(torch, plan, batch, got):
    name = "ii65"
    mtr, take = batch["mtr"], batch["take"]
    d_rows, d_ref = batch["d_rows"][:, :, :N], batch["d_ref"][:, :N]
    full = got(name)
    # a repeated call
    again = call(plan, d_rows, d_ref, name, mtr=mtr)
    assert same(again["fit"], full["fit"]) and np.array_equal(again["lag"], full["lag"])
    # the batch against one-ensemble calls (B = 1 against B = 3)
    for b in range(B):
        one = call(plan, d_rows[b:b + 1], d_ref[b:b + 1], name, mtr=mtr[b:b + 1])
        assert same(one["fit"][0], full["fit"][b]) and np.array_equal(one["lag"][0], full["lag"][b]), b
    # a row of the M = 9 call against its M = 1 call
    for b, m in ((0, 0), (0, 8), (1, 2), (2, 6)):
        one = call(plan, d_rows[b:b + 1, m:m + 1], d_ref[b:b + 1], name)
        assert same(one["fit"][0, 0], full["fit"][b, m]) and np.array_equal(one["lag"][0, 0], full["lag"][b, m]), (b, m)
    # each range alone
    off = 0
    for w, (n0, n1) in enumerate(dr.RANGES):
        one = call(plan, d_rows, d_ref, name, mtr=mtr, ranges=((n0, n1),))
        assert same(one["fit"][:, :, 0], full["fit"][:, :, w]) and np.array_equal(one["lag"], full["lag"][:, :, off:off + n1 - n0]), w
        off += n1 - n0
    # without the lags
    assert same(call(plan, d_rows, d_ref, name, mtr=mtr, lag=False), full["fit"])
    # the view of the padded base against a contiguous copy
    copy = call(plan, d_rows.contiguous(), d_ref.contiguous(), name, mtr=mtr)
    assert same(copy["fit"], full["fit"]) and np.array_equal(copy["lag"], full["lag"])
    # every row taking part: the rows that did before keep their bits
    allin = call(plan, d_rows, d_ref, name)
    assert same(allin["fit"][take], full["fit"][take]) and np.array_equal(allin["lag"][take], full["lag"][take])
    assert (allin["fit"][~take][:, (1, 2, 3)][..., 5] >= 0).any()


def test_small_budget_takes_rounds_bit_identically(torch, tmp_path):
    """The rounds batch under TSPWS_PART_MB=16 in a child process (3 rounds) against the one-round outputs of this process, bit for bit."""
    fit, lag, st = dc.run(torch)
    Lmax, _ = dr.SETS["iii"]
    assert st == dict(rounds=1, rows=dc.RB * dc.RM - 6, left_out=6, lags=2 * Lmax + 1, samples=T), st
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "dtw_rows_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "DTW_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) == 3, int(small["rounds"])
    assert same(small["fit"], fit) and np.array_equal(small["lag"], lag)
    assert (lag[5, ::4] == dr.INT_MIN).all() and (lag[5, 1] != dr.INT_MIN).all() and (fit[5, ::4, :, 5] == -1).all() and (fit[11, :, 0, 5] >= 0).all()


def test_hygiene(torch, lib, plan, batch, got):
    """Through the C entry point on outputs with 64 spare values behind each: nothing past [B][M][W][6] and [B][M][T] is written, the
    inputs are unchanged, empty inputs do nothing."""
    import ctypes as C
    name = "iii"
    Lmax, b = dr.SETS[name]
    full = got(name)
    o_fit = torch.full((B * M * W * 6 + 64,), -5.0, dtype=torch.float64, device="cuda")
    o_lag = torch.full((B * M * T + 64,), 77, dtype=torch.int32, device="cuda")
    cp = tspws.dtw_par(Lmax, b)
    wa = np.ascontiguousarray(np.array(dr.RANGES, dtype=np.uint64))
    mtr = batch["mtr"]
    rc = lib.tspws_hip_dtw_rows(plan.h, batch["d_rows"].data_ptr(), N + 3, B, M, mtr.ctypes.data, batch["d_ref"].data_ptr(), N + 1, dr.Z, C.addressof(cp),
                                wa.ctypes.data, W, o_lag.data_ptr(), o_fit.data_ptr(), None)
    assert rc == 0, lib.tspws_hip_last_error()
    hf, hl = o_fit.cpu().numpy(), o_lag.cpu().numpy()
    assert (hf[B * M * W * 6:] == -5.0).all() and (hl[B * M * T:] == 77).all()
    assert same(hf[:B * M * W * 6], full["fit"].reshape(-1)) and np.array_equal(hl[:B * M * T], full["lag"].reshape(-1))
    assert np.array_equal(batch["d_rows"].cpu().numpy(), batch["rows"], equal_nan=True) and np.array_equal(batch["d_ref"].cpu().numpy(), batch["ref"], equal_nan=True)
    empty = plan.dtw_rows(batch["d_rows"][:0, :, :N], batch["d_ref"][:0, :N], dr.Z, dict(Lmax=Lmax, b=b), dr.RANGES)
    assert tuple(empty["fit"].shape) == (0, M, W, 6) and tuple(empty["lag"].shape) == (0, M, T)


def test_recovery_and_sign(torch, plan):
    """dtw_rows_ref.recovery_rows: cur(t) = ref(t (1 +- 1e-2)) at z = 750, Lmax = 10, b = 4, on 600 samples of lag on either side.  The device
    equals the checker bit for bit, so the tolerance tests the method, not the kernel: per (row, range) it is the checker's own
    |eps_hat - eps| on this input plus the integer-lag quantisation 1 / (n_w sqrt(12)) = 4.8e-4 (dtw_rows_ref.recovery_tolerance).  The
    checker's own error is at most a tenth of eps (test_dtw_rows_cpu.py).  eps_hat has the sign of stretch_rows' answer on the same rows."""
    ref, rows = dr.recovery_rows()
    tol, eh = dr.recovery_tolerance()
    d_rows, d_ref = torch.from_numpy(rows[None]).cuda(), torch.from_numpy(ref[None]).cuda()
    out = plan.dtw_rows(d_rows, d_ref, dr.Z, dict(Lmax=dr.RLMAX, b=dr.RB), dr.RRANGES)
    fit = out["fit"].cpu().numpy()
    sfit = plan.stretch_rows(d_rows, d_ref, dr.Z, tspws.stretch_grid(0.03, 201), dr.RRANGES).cpu().numpy()
    for m, eps in enumerate((dr.REPS, -dr.REPS)):
        for w in range(len(dr.RRANGES)):
            print(f"row {m} range {w}: eps_hat {fit[0, m, w, 0]:+.6e} (checker {eh[m, w]:+.6e}, tolerance {tol[m, w]:.2e}), stretch_rows {sfit[0, m, w, 0]:+.6e}")
            assert fit[0, m, w, 0] == eh[m, w]
            assert abs(fit[0, m, w, 0] - eps) <= tol[m, w]
            assert np.sign(fit[0, m, w, 0]) == np.sign(sfit[0, m, w, 0]) == np.sign(eps)
