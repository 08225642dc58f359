"""GPU tests of the group-arrival calls (tspws_hip_ftan_coef, tspws_hip_ftan_rows), on the shipped library, against the checker
tests/ftan_rows_ref.py.

Parity: the batch of ftan_rows_ref.parity_batch (N = 1501, odd: the finest octave has D = 2, so 751 coefficients and 3 segments; ld = N + 3
with NaN pad columns; B = 3, M = 5 with counts that leave out 0 / 2 / 4 rows; W = 2 windows per ensemble whose edges are no multiples of
any D, ensembles 0 and 2 sharing their tables (one class) and ensemble 1 with others; a noise range per ensemble) at z = 750 and 750.25,
with and without the wrap rule, P = 1, 3, 4, all scales and a partial range.  The coefficient sets come from Plan.forward on the device and
are downloaded; the checker runs on those bits: the peaks bit for bit (NaN matching NaN), Q inside its any-order bound, n exact, the stats
from the definition.  Then ftan_rows against ftan_coef, the constructed sets through ftan_coef (uploaded, not transformed), the
independence properties bit for bit, three rounds under a small budget in a child process, the recovery of known group arrivals, the
refusals that need a plan, and the outputs' hygiene."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import ftan_rows_child as ftc
import ftan_rows_ref as fr_

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N = fr_.N
B, M, W = fr_.B, fr_.M, 2
NAN = float("nan")
same = fr_.same


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
    return fr_.Frame.from_plan(plan)


@pytest.fixture(scope="module")
def batch(torch, plan):
    """The parity batch with its device coefficient sets, downloaded once: dict(rows, mtr (host), d_rows, Y (device), hY (host), ens)."""
    rows, mtr = fr_.parity_batch(0)
    d_rows = torch.from_numpy(rows).cuda()
    Y = plan.forward(d_rows.view(B * M, N + 3)[:, :N])
    hY = Y.cpu().numpy()
    assert np.isfinite(hY).all()
    return dict(rows=rows, mtr=mtr, d_rows=d_rows, Y=Y, hY=hY, ens=np.arange(B * M, dtype=np.uint32) // M)


@pytest.fixture(scope="module")
def full(plan, batch):
    """(peaks, noise) of ftan_rows on the parity batch at z = 750, P = 4, all scales, without the wrap rule, as numpy: what the independence
    tests compare against."""
    peaks, nz = plan.ftan_rows(batch["d_rows"][:, :, :N], fr_.Z, fr_.PWIN, P=4, noise=fr_.PNOISE, mtr=batch["mtr"])
    return peaks.cpu().numpy(), nz.cpu().numpy()


@pytest.mark.parametrize("P,scales", ((4, None), (3, (3, 23)), (1, None)))
@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("z", fr_.ZS)
def test_parity(plan, frame, batch, z, skip, P, scales):
    rows = batch["rows"]
    assert np.isnan(rows[:, :, N:]).all() and np.isfinite(rows[:, :, :N]).all()
    sc = scales or (0, plan.S)
    Sx = sc[1] - sc[0]
    peaks, nz = plan.ftan_coef(batch["Y"], z, fr_.PWIN, scales=scales, P=P, noise=fr_.PNOISE, ens=batch["ens"], B=B, skip_wrapped=skip)
    st = plan.ftan_rows_stats()
    peaks, nz = peaks.cpu().numpy(), nz.cpu().numpy()
    assert peaks.shape == (B * M, W, Sx, P, 5) and nz.shape == (B * M, Sx, 2)
    want = fr_.reference(frame, batch["hY"], z, fr_.PWIN, sc, P, ens=batch["ens"], skip_wrapped=skip, noise=fr_.PNOISE)
    what = f"z = {z} skip_wrapped = {skip} P = {P} scales = {sc}"
    found = int((want["peaks"][..., 4] >= 0).sum())
    print(what, ": peaks", found, "of", want["peaks"][..., 4].size, "slots")
    assert same(peaks, want["peaks"]), what
    fr_.check_noise(nz, want, what)
    assert st == fr_.expected_stats(frame, fr_.PWIN, fr_.PNOISE, sc, skip, B, B * M, 0), st
    assert st["classes"] == 2
    # the segments of the finest scales are exercised (a property of the inputs), and both full and short lists occur
    assert fr_.members(frame, sc[0], fr_.PWIN[1, 1], False).size > 512
    assert found > 0 and (P == 1 or (want["peaks"][..., 4] < 0).any())


def test_rows_equal_coef(plan, frame, batch):
    mtr = batch["mtr"]
    for z, skip in ((750.0, False), (750.25, True)):
        peaks, nz = plan.ftan_rows(batch["d_rows"][:, :, :N], z, fr_.PWIN, P=3, noise=fr_.PNOISE, mtr=mtr, skip_wrapped=skip)
        st = plan.ftan_rows_stats()
        assert st == fr_.expected_stats(frame, fr_.PWIN, fr_.PNOISE, (0, plan.S), skip, B, 5 + 3 + 1, 6), st
        peaks, nz = peaks.cpu().numpy(), nz.cpu().numpy()
        assert peaks.shape == (B, M, W, plan.S, 3, 5) and nz.shape == (B, M, plan.S, 2)
        c_peaks, c_nz = plan.ftan_coef(batch["Y"], z, fr_.PWIN, P=3, noise=fr_.PNOISE, ens=batch["ens"], B=B, skip_wrapped=skip)
        c_peaks, c_nz = c_peaks.cpu().numpy().reshape(peaks.shape), c_nz.cpu().numpy().reshape(nz.shape)
        take = mtr > 0
        assert take.sum() == 9
        assert same(peaks[take], c_peaks[take]) and same(nz[take], c_nz[take])
        assert np.isnan(peaks[~take][..., :4]).all() and (peaks[~take][..., 4] == -1).all()
        assert np.isnan(nz[~take][..., 0]).all() and (nz[~take][..., 1] == -1).all()
        # without h_ens: row i is ensemble i
        one = plan.ftan_coef(batch["Y"][5:8], z, fr_.PWIN, P=2, skip_wrapped=skip).cpu().numpy()
        two = plan.ftan_coef(batch["Y"][5:8], z, fr_.PWIN, P=2, ens=np.arange(3, dtype=np.uint32), skip_wrapped=skip).cpu().numpy()
        assert same(one, two)
        # without the noise output the noise range is not needed
        assert same(plan.ftan_rows(batch["d_rows"][:, :, :N], z, fr_.PWIN, P=3, mtr=mtr, skip_wrapped=skip).cpu().numpy(), peaks)


def test_constructed_sets(torch, plan, frame):
    Y, win, noise, want = fr_.constructed(frame)
    d_Y = torch.from_numpy(Y).cuda()
    ens = np.zeros(len(Y), np.uint32)
    for P in (4, 3, 1):
        for skip in (False, True):
            peaks, nz = plan.ftan_coef(d_Y, fr_.Z, win, scales=(0, 3), P=P, noise=noise, ens=ens, B=1, skip_wrapped=skip)
            peaks, nz = peaks.cpu().numpy(), nz.cpu().numpy()
            ref = fr_.reference(frame, Y, fr_.Z, win, (0, 3), P, ens=ens, skip_wrapped=skip, noise=noise)
            for i, name in enumerate(fr_.CNAMES):
                assert same(peaks[i], ref["peaks"][i]), (name, P, skip, peaks[i, :, fr_.CS, :, 4], ref["peaks"][i, :, fr_.CS, :, 4])
            fr_.check_noise(nz, ref, f"constructed P = {P} skip_wrapped = {skip}")
            assert (nz[fr_.CNAMES.index("zero"), :, 0] == 0).all() and nz[fr_.CNAMES.index("equal"), fr_.CS, 0] == 70  # (exact in any order)
            if not skip:  # the lists the sets were built for (the checker's own test holds it to them on the CPU)
                for i, name in enumerate(fr_.CNAMES):
                    assert peaks[i, 0, fr_.CS, :, 4].tolist() == (want[name] + [-1] * 4)[:P], name
                    assert peaks[i, 1, fr_.CS, :, 4].tolist() == (fr_.CWHOLE.get(name, want[name]) + [-1] * 4)[:P], name
    i = fr_.CNAMES.index("inf_nan")
    assert not np.isfinite(Y[i]).all() and nz[i, 0, 1] == fr_.members(frame, fr_.CS, noise, True).size - 2


def test_independence(torch, plan, batch, full):
    mtr = batch["mtr"]
    d_rows = batch["d_rows"][:, :, :N]
    peaks0, nz0 = full
    S = plan.S

    def run(r, win=fr_.PWIN, noise=fr_.PNOISE, m=None, P=4, scales=None):
        got = plan.ftan_rows(r, fr_.Z, win, scales=scales, P=P, noise=noise, mtr=m)
        return got[0].cpu().numpy(), got[1].cpu().numpy()

    # a repeated call
    p, q = run(d_rows, m=mtr)
    assert same(p, peaks0) and same(q, nz0)
    # the batch against a loop of one-ensemble calls
    for b in range(B):
        p, q = run(d_rows[b:b + 1], win=fr_.PWIN[b:b + 1], noise=fr_.PNOISE[b:b + 1], m=mtr[b:b + 1])
        assert same(p[0], peaks0[b]) and same(q[0], nz0[b]), b
    # a row of the M = 5 call against the M = 1 call on that row
    for b, m in ((0, 0), (0, 4), (1, 2), (2, 3)):
        p, q = run(d_rows[b:b + 1, m:m + 1], win=fr_.PWIN[b:b + 1], noise=fr_.PNOISE[b:b + 1])
        assert same(p[0, 0], peaks0[b, m]) and same(q[0, 0], nz0[b, m]), (b, m)
    # each window alone
    for w in range(W):
        p, q = run(d_rows, win=fr_.PWIN[:, w:w + 1], m=mtr)
        assert same(p[:, :, 0], peaks0[:, :, w]) and same(q, nz0), w
    # a sub-range of scales against its slots of the full range
    p, q = run(d_rows, m=mtr, scales=(5, 17))
    assert same(p, peaks0[:, :, :, 5:17]) and same(q, nz0[:, :, 5:17])
    p, q = run(d_rows, m=mtr, scales=(S - 1, S))
    assert same(p, peaks0[:, :, :, S - 1:]) and same(q, nz0[:, :, S - 1:])
    # P = 2 and P = 1 as the head of P = 4
    for P in (2, 1):
        p, q = run(d_rows, m=mtr, P=P)
        assert same(p, peaks0[..., :P, :]) and same(q, nz0), P
    # the view of the padded base against a contiguous copy
    p, q = run(d_rows.contiguous(), m=mtr)
    assert same(p, peaks0) and same(q, nz0)
    # a (W, 2) window table and one noise pair are every ensemble's
    p, q = run(d_rows, win=fr_.PWIN[1], noise=fr_.PNOISE[1], m=mtr)
    assert same(p[1], peaks0[1]) and same(q[1], nz0[1]) and plan.ftan_rows_stats()["classes"] == 1


def test_small_budget_takes_rounds_bit_identically(torch, tmp_path):
    """The rounds batch under TSPWS_PART_MB=16 in a child process (3 rounds) against the one-round outputs of this process, bit for bit."""
    peaks, nz, st = ftc.run(torch)
    assert st["rounds"] == 1 and st["rows"] == ftc.RB * ftc.RM - 3 and st["left_out"] == 3 and st["classes"] == 2, st
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "ftan_rows_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "FTAN_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2, int(small["rounds"])
    assert same(small["peaks"], peaks) and same(small["noise"], nz)
    assert (peaks[2, :, :, :, 0, 4] >= 0).any() and (peaks[5, ::4, ..., 4] == -1).all() and (peaks[5, 1, ..., 0, 4] >= 0).any()


def test_recovery(torch):
    """The group arrivals of Gaussian wave packets at the scales 4, 8, .., 24 (N = 4096, default frame, z = 2048): |tg + z - t0| <= 0.25 D_s,
    and bit equality with the checker on the device's sets."""
    pl = tspws.Plan(tspws.resolve(abi.default_params(), fr_.RN), fr_.RN)
    fr = fr_.Frame.from_plan(pl)
    assert fr.S == 36
    row, t0s = fr_.recovery_row(fr)
    d_row = torch.from_numpy(row[None, None]).cuda()
    hY = pl.forward(d_row[0]).cpu().numpy()
    peaks = pl.ftan_rows(d_row, fr_.RZ, fr_.RWIN, P=1).cpu().numpy()
    assert peaks.shape == (1, 1, 1, 36, 1, 5)
    want = fr_.reference(fr, hY, fr_.RZ, fr_.RWIN, (0, 36), 1)["peaks"]
    assert same(peaks[0], want)
    fr_.check_recovery(fr, peaks[0, :, 0], t0s, "device")


def test_refusals_and_hygiene(torch, lib, plan, batch, full):
    d_rows, mtr = batch["d_rows"], batch["mtr"]
    S = plan.S
    npk, nnz = B * M * W * S * 4 * 5, B * M * S * 2
    o_peaks = torch.full((npk + 64,), NAN, dtype=torch.float64, device="cuda")
    o_nz = torch.full((nnz + 64,), NAN, dtype=torch.float64, device="cuda")
    o_peaks[-64:] = 7.0
    o_nz[-64:] = 7.0
    got = plan.ftan_rows(d_rows[:, :, :N], fr_.Z, fr_.PWIN, P=4, noise=fr_.PNOISE, mtr=mtr, out=(o_peaks, o_nz))
    assert got[0] is o_peaks and got[1] is o_nz
    h_peaks, h_nz = o_peaks.cpu().numpy(), o_nz.cpu().numpy()
    assert (h_peaks[-64:] == 7.0).all() and (h_nz[-64:] == 7.0).all()  # nothing past [B][M][W][S][P][5] / [B][M][S][2]
    assert same(h_peaks[:-64].reshape(full[0].shape), full[0]) and same(h_nz[:-64].reshape(full[1].shape), full[1])
    # the inputs are unchanged (NaN pads included)
    assert np.array_equal(d_rows.cpu().numpy(), batch["rows"], equal_nan=True)
    # empty inputs do nothing
    assert tuple(plan.ftan_rows(d_rows[:0, :, :N], fr_.Z, fr_.PWIN[0], P=2).shape) == (0, M, W, S, 2, 5)

    # what only the plan can judge, through the C entry points on sentinel-filled outputs
    s_peaks = torch.full((npk,), -3.0, dtype=torch.float64, device="cuda")
    s_nz = torch.full((nnz,), -4.0, dtype=torch.float64, device="cuda")
    wa, na = np.ascontiguousarray(fr_.PWIN, dtype=np.uint64), np.ascontiguousarray(fr_.PNOISE, dtype=np.uint64)

    def untouched():
        torch.cuda.synchronize()
        assert bool((s_peaks == -3.0).all()) and bool((s_nz == -4.0).all())  # outputs untouched
        return lib.tspws_hip_last_error()

    def rows_call(ld=N + 3, wa=wa, na=na, nb=B, m=M, sc=(0, S), P=4):
        rc = lib.tspws_hip_ftan_rows(plan.h, d_rows.data_ptr(), ld, nb, m, None, fr_.Z, sc[0], sc[1], wa.ctypes.data, wa.shape[1], na.ctypes.data, P, 0,
                                     s_peaks.data_ptr(), s_nz.data_ptr(), None)
        return rc, untouched()

    def coef_call(ens=None, nrow=B * M, nb=B, wa=wa, na=na, sc=(0, S), P=4):
        e = None if ens is None else np.ascontiguousarray(ens, dtype=np.uint32)
        rc = lib.tspws_hip_ftan_coef(plan.h, batch["Y"].data_ptr(), None if e is None else e.ctypes.data, nrow, nb, fr_.Z, sc[0], sc[1], wa.ctypes.data,
                                     wa.shape[1], na.ctypes.data, P, 0, s_peaks.data_ptr(), s_nz.data_ptr(), None)
        return rc, untouched()

    past_w, past_n = wa.copy(), na.copy()
    past_w[2, 1, 1] = N + 1
    past_n[1, 1] = N + 1
    ens = batch["ens"]
    assert rows_call(ld=N - 1) == (-1, b"ftan_rows: row stride below the trace length")
    for who, fn, kw in ((b"ftan_rows: ", rows_call, dict()), (b"ftan_coef: ", coef_call, dict(ens=ens))):
        assert fn(sc=(0, S + 1), **kw) == (-1, who + b"the scale range ends behind the last scale")
        assert fn(wa=past_w, **kw) == (-1, who + b"a window past the trace length")
        assert fn(na=past_n, **kw) == (-1, who + b"a noise range past the trace length")
        # what needs no plan is refused with one, too
        assert fn(sc=(4, 4), **kw) == (-1, who + b"an empty scale range (s_begin >= s_end)")
        assert fn(P=5, **kw) == (-1, who + b"1 to 4 peaks")
        assert fn(P=0, **kw) == (-1, who + b"1 to 4 peaks")
    bad = ens.copy()
    bad[-1] = B
    assert coef_call(ens=bad) == (-1, b"ftan_coef: an ensemble index >= B")
    assert coef_call(ens=None) == (-1, b"ftan_coef: without h_ens the rows must number B")
    # more than 2^32 - 16 rows: refused from the counts alone, before any row or table is looked at
    assert rows_call(nb=0x10000, m=0x10000) == (-1, b"ftan_rows: more than 2^32 - 16 rows")
    assert coef_call(ens=None, nrow=0xfffffff1, nb=0xfffffff1) == (-1, b"ftan_coef: more than 2^32 - 16 rows")
    # B == 0, M == 0, nrow == 0: nothing happens
    assert rows_call(nb=0)[0] == 0 and rows_call(m=0)[0] == 0 and coef_call(ens=ens, nrow=0)[0] == 0 and coef_call(ens=ens, nb=0)[0] == 0
    # d_noise without h_noise
    rc = lib.tspws_hip_ftan_rows(plan.h, d_rows.data_ptr(), N + 3, B, M, None, fr_.Z, 0, S, wa.ctypes.data, W, None, 4, 0, s_peaks.data_ptr(), s_nz.data_ptr(), None)
    assert (rc, untouched()) == (-1, b"ftan_rows: a noise output without a noise range")
    with pytest.raises(tspws.TspwsError, match="ftan_rows: a window past the trace length"):
        plan.ftan_rows(d_rows[:, :, :N], fr_.Z, ((0, N + 1),))
    with pytest.raises(tspws.TspwsError, match="ftan_coef: 1 to 4 windows"):
        plan.ftan_coef(batch["Y"], fr_.Z, [(0, 10)] * 5, ens=ens, B=B)
    with pytest.raises(tspws.TspwsError, match="windows must be"):
        plan.ftan_rows(d_rows[:, :, :N], fr_.Z, fr_.PWIN[:2])
