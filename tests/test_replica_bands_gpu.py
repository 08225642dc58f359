"""Percentile bands over replica rows (tspws_hip_replica_bands, Plan.replica_bands) on the GPU, shipped library, against the numpy checker
tests/replica_bands_ref.py: the parity batch (N = 1501: a partial last tile; ld = N + 3 with NaN pad columns; scales of 1e-6 .. 1e2, a
constant, a tie and a +-0 column, one +inf and one -inf entry) with and without a count table; both routes on either side of
lds_max_rows; the bands of real bootstrap replicas; hygiene (a repeated call, guard blocks, out=, a side stream, empty inputs, refusals);
and two rounds under a small budget in a child process.  Every comparison with the checker is np.array_equal(..., equal_nan=True): bit
equality up to the sign of zero, no sample excused."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import replica_bands_child as rbc
import replica_bands_ref as rbr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
N, PAD, B = 1501, 3, 6
QS = [0, 0.025, 0.16, 1 / 3, 0.5, 0.84, 0.975, 1]
NAN = float("nan")


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


def bands_of(torch, plan, base, q, mtr):
    """Plan.replica_bands on the [B][M][:N] view of a padded base, into a NaN-filled output; (bands as numpy, stats)."""
    dev = torch.from_numpy(base).cuda()
    out = torch.full((base.shape[0], len(q), N), NAN, dtype=torch.float32, device="cuda")
    got = plan.replica_bands(dev[:, :, :N], q, mtr, out=out)
    assert got is out
    return out.cpu().numpy(), plan.replica_bands_stats()


@pytest.mark.parametrize("counted", [False, True], ids=["all", "counts"])
@pytest.mark.parametrize("q", [QS, [0.5]], ids=["Q8", "Q1"])
@pytest.mark.parametrize("M", [1, 2, 9, 100, 101])
def test_parity(lib, torch, plan, M, q, counted):
    base = rbr.parity_rows(B, M, N, N + PAD, seed=M)
    assert np.isnan(base[:, :, N:]).all() and np.isfinite(np.delete(base[:, :, :N], [11, 13], axis=2)).all()
    mtr = rbr.parity_counts(B, M, seed=M) if counted else None
    got, st = bands_of(torch, plan, base, q, mtr)
    want = rbr.expected(base[:, :, :N], q, mtr)
    finite = np.delete(got, [11, 13], axis=2)  # the columns of the two infinities aside, every input is finite (the NaN pad is never read)
    assert np.isfinite(finite).all()
    assert np.array_equal(got, want, equal_nan=True), int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
    assert np.abs(np.delete(want, [11, 13], axis=2)).max() > 0
    if counted:
        assert st["lds"] == B - 1 and st["empty"] == 1 and st["global"] == 0 and st["rounds"] == 1, st
        assert not got[1].any()                                   # every count 0: zero bands
        for k in range(len(q)):                                   # exactly one count > 0: that row for every q
            assert np.array_equal(got[2, k], base[2, M // 2, :N], equal_nan=True)
    else:
        assert st["lds"] == B and st["empty"] == 0 and st["global"] == 0 and st["rounds"] == 1, st


def test_both_routes_by_size(lib, torch, plan):
    """M = lds_max_rows takes the LDS route, M + 1 the columns in global memory; both equal the checker."""
    bands_of(torch, plan, rbr.parity_rows(1, 2, N, N, seed=1), [0.5], None)  # a first call
    L = plan.replica_bands_stats()["lds_max_rows"]
    assert 64 <= L <= 640, L  # (a workgroup's LDS is 160 KiB, a row of a 64-sample tile 256 bytes)
    q = [0.025, 0.5, 0.975]
    for M, route in ((L, "lds"), (L + 1, "global")):
        base = rbr.parity_rows(2, M, N, N + PAD, seed=M)
        got, st = bands_of(torch, plan, base, q, None)
        assert st[route] == 2 and st["lds"] + st["global"] == 2 and st["empty"] == 0, (M, st)
        assert np.array_equal(got, rbr.expected(base[:, :, :N], q, None), equal_nan=True), M


def test_on_real_replicas(lib, torch):
    """The bands of the rows Plan.bootstrap_batch leaves (tests/boot_batch_engine.py's batch, M = 17: an empty ensemble, an all-zero count row)."""
    import boot_batch_engine as bbe
    r = bbe.run(torch, "morlet1501", "unbiased", bbe.counts())
    bbe.check_counts(r)
    pl, mtr = r["pl"], r["sm"]
    assert mtr.shape == (len(bbe.SIZES), bbe.MMAX) and not mtr[4].any() and not mtr[:, bbe.ROW_ZERO].any()
    for k in ("sl", "st"):
        rows = torch.from_numpy(r[k]).cuda()
        got = pl.replica_bands(rows, QS, mtr)
        st = pl.replica_bands_stats()
        assert st["lds"] == 5 and st["empty"] == 1 and st["global"] == 0, st
        g = got.cpu().numpy()
        assert np.array_equal(g, rbr.expected(r[k], QS, mtr), equal_nan=True), k
        assert np.isfinite(g).all() and (np.diff(g, axis=1) >= 0).all(), k  # non-decreasing in q at every sample
        assert not g[4].any()                                              # the empty ensemble
        for b in (0, 1, 2, 3, 5):
            take = torch.from_numpy(mtr[b] > 0).cuda()
            assert not bool(take[bbe.ROW_ZERO]) and int(take.sum()) == bbe.MMAX - 1
            assert torch.equal(got[b, 0], torch.amin(rows[b][take], dim=0)) and torch.equal(got[b, -1], torch.amax(rows[b][take], dim=0)), (k, b)
        # ... and the all-zero row would show if it took part: without the counts the extremes differ somewhere
        every = pl.replica_bands(rows, QS, None).cpu().numpy()
        assert not np.array_equal(every[:, [0, -1]], g[:, [0, -1]])


def test_hygiene(lib, torch, plan):
    M, Q = 9, len(QS)
    base = rbr.parity_rows(B, M, N, N + PAD, seed=77)
    mtr = rbr.parity_counts(B, M, seed=77)
    want = rbr.expected(base[:, :, :N], QS, mtr)
    dev = torch.from_numpy(base).cuda()
    rows = dev[:, :, :N]
    # guard blocks before and after the bands stay intact; a repeated call is bit-identical
    G, n = 4096, B * Q * N
    block = torch.full((G + n + G,), NAN, dtype=torch.float32, device="cuda")
    out = block[G:G + n].view(B, Q, N)
    assert plan.replica_bands(rows, QS, mtr, out=out) is out
    a = out.cpu().numpy().copy()
    assert np.array_equal(a, want, equal_nan=True)
    assert bool(torch.isnan(block[:G]).all()) and bool(torch.isnan(block[G + n:]).all())
    out.fill_(NAN)
    plan.replica_bands(rows, QS, mtr, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert bool(torch.isnan(block[:G]).all()) and bool(torch.isnan(block[G + n:]).all())
    # without out= a new tensor; a contiguous [B][M][N] tensor gives the same bands
    fresh = plan.replica_bands(rows.contiguous(), QS, mtr)
    assert fresh.shape == (B, Q, N) and fresh.dtype == torch.float32 and np.array_equal(fresh.cpu().numpy().view(np.uint32), a.view(np.uint32))
    # a call on a non-default stream returns with the bands complete: another stream reads them without waiting for the first
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    side = torch.full((B, Q, N), NAN, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        plan.replica_bands(rows, QS, mtr, out=side)
    with torch.cuda.stream(s2):
        seen = side.cpu().numpy()
    assert np.array_equal(seen.view(np.uint32), a.view(np.uint32))
    # what the binding refuses
    for bad in (dict(out=torch.zeros((B, Q, N + 1), dtype=torch.float32, device="cuda")), dict(out=torch.zeros((B, Q + 1, N), dtype=torch.float32, device="cuda")),
                dict(out=torch.zeros((B, Q, N), dtype=torch.float64, device="cuda")), dict(mtr=mtr.astype(np.int64)), dict(mtr=mtr[:, :-1]),
                dict(rows=dev), dict(rows=rows.double()), dict(rows=rows.cpu()), dict(rows=rows[0]), dict(q=[[0.5]]), dict(q="median")):
        kw = dict(rows=rows, q=QS, mtr=mtr, out=None)
        kw.update(bad)
        with pytest.raises(tspws.TspwsError):
            plan.replica_bands(kw["rows"], kw["q"], kw["mtr"], out=kw["out"])
    with pytest.raises(tspws.TspwsError, match="replica_bands: a probability"):
        plan.replica_bands(rows, [0.5, 1.5], mtr)
    with pytest.raises(tspws.TspwsError, match="replica_bands: more than 8"):
        plan.replica_bands(rows, [0.1] * 9, mtr)


def test_empty_inputs_and_refusals_with_a_plan(lib, torch, plan):
    M = 3
    rows = torch.zeros((2, M, N), dtype=torch.float32, device="cuda")
    out = torch.full((2 * 8 * N,), -3.0, dtype=torch.float32, device="cuda")
    mtr = np.ones((2, M), np.uint32)

    def cabi(pl=plan.h, r=True, q=(0.025, 0.5), Q=None, o=True, qptr=True, Bn=2, Mn=M, ld=N, m=True):
        qa = np.array(q, dtype=np.float64)
        rc = lib.tspws_hip_replica_bands(pl, rows.data_ptr() if r else None, ld, Bn, Mn, mtr.ctypes.data if m else None, qa.ctypes.data if qptr else None,
                                         qa.size if Q is None else Q, out.data_ptr() if o else None, None)
        torch.cuda.synchronize()
        assert bool((out == -3.0).all())  # outputs untouched
        return rc, lib.tspws_hip_last_error()

    for kw in (dict(Bn=0), dict(Mn=0), dict(Q=0), dict(Q=0, qptr=False)):
        assert cabi(**kw)[0] == 0, kw
    for kw in (dict(pl=None), dict(r=False), dict(qptr=False), dict(o=False)):
        rc, err = cabi(**kw)
        assert rc == -1 and b"replica_bands: NULL" in err, (kw, err)
    rc, err = cabi(ld=N - 1)
    assert rc == -1 and b"replica_bands: row stride" in err, err
    rc, err = cabi(q=[0.1] * 9)
    assert rc == -1 and b"replica_bands: more than 8" in err, err
    for bad in (NAN, -1e-9, 1.0000001, float("inf")):
        rc, err = cabi(q=[bad, 0.5])
        assert rc == -1 and b"replica_bands: a probability outside" in err, (bad, err)
    # ... and the same shapes through the binding: nothing to do, the sentinel stays
    o = torch.full((2, 2, N), -3.0, dtype=torch.float32, device="cuda")
    assert plan.replica_bands(rows[:, :0], [0.1, 0.9], None, out=o) is o and bool((o == -3.0).all())
    assert tuple(plan.replica_bands(rows[:0], [0.1, 0.9]).shape) == (0, 2, N) and tuple(plan.replica_bands(rows, []).shape) == (2, 0, N)
    # the call that is not refused writes
    half = np.array([0.5])
    rc = lib.tspws_hip_replica_bands(plan.h, rows.data_ptr(), N, 2, M, None, half.ctypes.data, 1, out.data_ptr(), None)
    assert rc == 0 and bool((out[:2 * N] == 0).all()) and bool((out[2 * N:] == -3.0).all())


def test_small_budget_takes_rounds_bit_identically(lib, torch, tmp_path):
    """The 17 MB batch under TSPWS_PART_MB=16 in a child process (2 rounds) against the one-round bands of this process, bit for bit."""
    one, st = rbc.run(torch)
    assert st["rounds"] == 1 and st["lds"] == rbc.B - 1 and st["empty"] == 1, st
    rows, mtr = rbc.batch()
    assert np.array_equal(one, rbr.expected(rows, rbc.QS, mtr), equal_nan=True)
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "replica_bands_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "BANDS_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2
    assert np.isfinite(one).all() and np.array_equal(small["bands"].view(np.uint32), one.view(np.uint32))
