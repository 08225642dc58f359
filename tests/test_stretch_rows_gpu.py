"""GPU tests of the stretching call (tspws_hip_stretch_rows), on the shipped library, against the checker tests/stretch_rows_ref.py.

Parity: the batch of tests/stretch_rows_child.py (N = 1501; ld = N + 3 and ldr = N + 1 with NaN pad columns; B = 3, M = 33 with counts that
leave out 0 / 16 / 32 rows; E = 41; the three windows, whose edges are no multiples of 4 and one of which touches both ends; noise of sigma
0, 0.2, 1; scales of 1e-6 .. 1e2; an all-zero row; a reference that is zero inside a window) at z = 750, 0 and 750.25: every cc inside the
checker's bound, NaN exactly where the checker has NaN, the fit bit for bit the contract's formula on the library's own cc, e* the checker's
argmax.  The seed is the first one for which no row's two largest cc* are closer than the sum of their bounds, at all three z: a condition
on the inputs, found on the CPU.  Then recovery of a known stretch, the independence properties bit for bit, two rounds and several grid
chunks under a small budget in a child process, and the outputs' hygiene."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import stretch_rows_child as src
import stretch_rows_ref as srr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N = srr.N
ZS = (750.0, 0.0, 750.25)
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
def eps(lib):
    return tspws.stretch_grid(0.01, 41)


@pytest.fixture(scope="module")
def batch(eps):
    """The parity batch of the first seed whose margins hold at every z, with the checker's answers: computed once, never changed."""
    for seed in range(20):
        rows, ref, mtr = src.parity_batch(seed)
        want = {z: srr.reference(rows[:, :, :N], ref[:, :N], z, eps, srr.WINDOWS, mtr) for z in ZS}
        if all(srr.margins_ok(w) for w in want.values()):
            print("parity batch: seed", seed)
            return rows, ref, mtr, want
    raise AssertionError("no seed in 0 .. 19 separates every row's two largest cc*")


@pytest.fixture(scope="module")
def dev(torch, batch):
    rows, ref, mtr, _ = batch
    return torch.from_numpy(rows).cuda(), torch.from_numpy(ref).cuda()


@pytest.fixture(scope="module")
def full(plan, dev, batch, eps):
    """(cc, fit) of the parity batch at z = 750 as numpy: what the independence tests compare against."""
    cc, fit = plan.stretch_rows(dev[0][:, :, :N], dev[1][:, :N], srr.Z, eps, srr.WINDOWS, mtr=batch[2], cc=True)
    return cc.cpu().numpy(), fit.cpu().numpy()


@pytest.mark.parametrize("z", ZS)
def test_parity(plan, dev, batch, eps, z):
    rows, ref, mtr, want = batch
    assert np.isnan(rows[:, :, N:]).all() and np.isnan(ref[:, N:]).all() and np.isfinite(rows[:, :, :N]).all() and np.isfinite(ref[:, :N]).all()
    cc, fit = plan.stretch_rows(dev[0][:, :, :N], dev[1][:, :N], z, eps, srr.WINDOWS, mtr=mtr, cc=True)
    cc, fit = cc.cpu().numpy(), fit.cpu().numpy()
    st = plan.stretch_rows_stats()
    assert st == dict(rounds=1, segments=7, rows=33 + 17 + 1, left_out=48, chunks=1), st
    w = want[z]
    srr.check(cc, w, f"z = {z}")
    out = mtr == 0
    assert np.isnan(cc[out]).all() and np.isnan(fit[out][:, :, :2]).all() and (fit[out][:, :, 2] == -1).all() and (fit[out][:, :, 3] == 1).all()
    assert np.isnan(cc[0, 5]).all() and (fit[0, 5, :, 2] == -1).all()  # the all-zero row
    assert not np.isnan(cc[~out & ~((np.arange(3)[:, None] == 0) & (np.arange(33)[None, :] == 5))][:, 2]).any()  # live rows, whole-trace window
    assert np.isnan(cc[1, ::2, 0, 20]).all()  # the dead stretched reference: eps = 0 leaves ensemble 1's reference as it is, zero in window 0
    assert same(fit, srr.fit(cc, eps))
    assert np.array_equal(fit[..., 2].astype(np.int64), w["argmax"])


def test_recovery(torch, plan, eps):
    ref, rows = srr.analytic_rows(0)
    fit = plan.stretch_rows(torch.from_numpy(rows[None]).cuda(), torch.from_numpy(ref[None]).cuda(), srr.Z, eps, srr.WINDOWS).cpu().numpy()
    step = eps[1] - eps[0]
    for j, e0 in enumerate(srr.EPS0):
        for w in range(len(srr.WINDOWS)):
            print(f"eps0 {e0:+.5f} window {srr.WINDOWS[w]}: eps_hat {fit[0, j, w, 0]:+.6f}, cc_hat {fit[0, j, w, 1]:.5f}")
            assert abs(fit[0, j, w, 0] - e0) <= step / 2 and fit[0, j, w, 1] >= 0.99 and fit[0, j, w, 3] == 0


def test_independence(torch, plan, dev, batch, eps, full):
    rows, ref, mtr, _ = batch
    d_rows, d_ref = dev[0][:, :, :N], dev[1][:, :N]
    cc0, fit0 = full

    def run(r, f, e=eps, wins=srr.WINDOWS, m=None, cc=True):
        got = plan.stretch_rows(r, f, srr.Z, e, wins, mtr=m, cc=cc)
        return (got[0].cpu().numpy(), got[1].cpu().numpy()) if cc else got.cpu().numpy()

    # a repeated call
    cc, fit = run(d_rows, d_ref, m=mtr)
    assert same(cc, cc0) and same(fit, fit0)
    # the batch against a loop of one-ensemble calls
    for b in range(3):
        cc, fit = run(d_rows[b:b + 1], d_ref[b:b + 1], m=mtr[b:b + 1])
        assert same(cc[0], cc0[b]) and same(fit[0], fit0[b]), b
    # a row of the M = 33 call against the M = 1 call on that row
    for b, m in ((0, 0), (0, 32), (1, 16), (2, 20)):
        cc, fit = run(d_rows[b:b + 1, m:m + 1], d_ref[b:b + 1])
        assert same(cc[0, 0], cc0[b, m]) and same(fit[0, 0], fit0[b, m]), (b, m)
    # a part of the grid against its columns of the full call
    cc, _ = run(d_rows, d_ref, e=eps[5:22], m=mtr)
    assert same(cc, cc0[..., 5:22])
    # each window alone against its slot
    for w, win in enumerate(srr.WINDOWS):
        cc, fit = run(d_rows, d_ref, wins=(win,), m=mtr)
        assert same(cc[:, :, 0], cc0[:, :, w]) and same(fit[:, :, 0], fit0[:, :, w]), w
    # without the cc output
    assert same(run(d_rows, d_ref, m=mtr, cc=False), fit0)
    # the view of the padded base against a contiguous copy
    cc, fit = run(d_rows.contiguous(), d_ref.contiguous(), m=mtr)
    assert same(cc, cc0) and same(fit, fit0)


def test_small_budget_takes_rounds_bit_identically(torch, tmp_path):
    """The rounds batch under TSPWS_PART_MB=16 in a child process (2 rounds; 4 and 2 chunks of the padded grid of 64) against the
    one-round, one-chunk outputs of this process, bit for bit."""
    cc, fit, st = src.run(torch)
    assert st["rounds"] == 1 and st["chunks"] == 1 and st["rows"] == src.RB * src.RM - 9 and st["left_out"] == 9, st
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "stretch_rows_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "STRETCH_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2 and int(small["chunks"]) >= 2, (int(small["rounds"]), int(small["chunks"]))
    assert same(small["cc"], cc) and same(small["fit"], fit)
    assert not np.isnan(cc[2]).any() and np.isnan(cc[5, ::4]).all() and not np.isnan(cc[5, 1]).any()


def test_outputs(torch, plan, dev, batch, eps, full):
    rows, ref, mtr, _ = batch
    B, M, W, E = 3, 33, 3, 41
    o_cc = torch.full((B * M * W * E + 64,), NAN, dtype=torch.float64, device="cuda")
    o_fit = torch.full((B * M * W * 4 + 64,), NAN, dtype=torch.float64, device="cuda")
    got = plan.stretch_rows(dev[0][:, :, :N], dev[1][:, :N], srr.Z, eps, srr.WINDOWS, mtr=mtr, cc=True, out=(o_cc, o_fit))
    assert got[0] is o_cc and got[1] is o_fit
    h_cc, h_fit = o_cc.cpu().numpy(), o_fit.cpu().numpy()
    assert np.isnan(h_cc[-64:]).all() and np.isnan(h_fit[-64:]).all()  # nothing past [B][M][W][E] / [B][M][W][4]
    assert same(h_cc[:-64].reshape(B, M, W, E), full[0]) and same(h_fit[:-64].reshape(B, M, W, 4), full[1])
    o_fit.fill_(NAN)
    got = plan.stretch_rows(dev[0][:, :, :N], dev[1][:, :N], srr.Z, eps, srr.WINDOWS, mtr=mtr, out=o_fit)
    assert got is o_fit and same(o_fit.cpu().numpy()[:-64].reshape(B, M, W, 4), full[1]) and np.isnan(o_fit.cpu().numpy()[-64:]).all()
    # the inputs are unchanged (NaN pads included)
    assert np.array_equal(dev[0].cpu().numpy(), rows, equal_nan=True) and np.array_equal(dev[1].cpu().numpy(), ref, equal_nan=True)
    # empty inputs do nothing; what only the plan can judge is refused with the call's text
    assert tuple(plan.stretch_rows(dev[0][:0, :, :N], dev[1][:0, :N], srr.Z, eps, srr.WINDOWS).shape) == (0, M, W, 4)
    with pytest.raises(tspws.TspwsError, match="stretch_rows: a window past the trace length"):
        plan.stretch_rows(dev[0][:, :, :N], dev[1][:, :N], srr.Z, eps, ((0, N + 1),))
