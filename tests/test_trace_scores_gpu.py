"""The trace scores (tspws_hip_trace_scores, Plan.trace_scores) on the GPU, shipped library, against the longdouble checker
tests/trace_scores_ref.py: every entry inside the checker's bounds (FP64 summation in any order; no tolerance chosen by hand), NaN
positions equal, the load route asserted through trace_scores_stats.  The scalar route (max = 1501), the vector route (max = 2048, also
through a padded base with NaN pad columns, and windows whose edges are no multiple of 4), three column segments with a ragged last one
(max = 8193: the smallest such length, scalar; max = 8196: the smallest on the vector route), traces and references without energy, the
float range, R = 1 .. 4, batch against loop, repeatability, guard cells, early returns, refusals, and two rounds under a small budget in a
child process."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import trace_scores_child as tsc
import trace_scores_ref as tsr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")
SIZES = (70, 0, 1)  # traces per ensemble; first[0] = 2
FIRST = 2 + np.concatenate([[0], np.cumsum(SIZES)])


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


_plans = {}


def plan_of(N):
    if N not in _plans:
        _plans[N] = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    return _plans[N]


_data = {}


def batch(N, R=2, pad=0):
    """(traces float32 [75][N + pad], refs float32 [3][R][N + pad]) of the standard batch, pad columns NaN: a common signal plus noise at
    scales 1e-3 .. 1e3, the references = signal plus their own noise; trace 9 and reference (0, R - 1) all zero, trace 11 scaled by 1e30
    and trace 12 by 1e-30.  The same values whatever the pad."""
    key = (N, R)
    if key not in _data:
        rng = np.random.default_rng(1000 + N + R)
        sig = np.sin(np.arange(N) * 0.05) * np.exp(-((np.arange(N) - N / 2) / (0.1 * N)) ** 2)
        x = (sig + rng.standard_normal((int(FIRST[-1]) + 2, N))) * 10.0 ** rng.uniform(-3, 3, (int(FIRST[-1]) + 2, 1))
        x = x.astype(np.float32)
        x[9] = 0
        x[11] *= np.float32(1e30) / np.abs(x[11]).max()
        x[12] *= np.float32(1e-30) / np.abs(x[12]).max()
        refs = (sig + 0.3 * rng.standard_normal((len(SIZES), R, N))).astype(np.float32)
        refs[0, R - 1] = 0
        _data[key] = (x, refs)
    x, refs = _data[key]
    if not pad:
        return x, refs
    xp = np.full((x.shape[0], N + pad), NAN, np.float32)
    rp = np.full(refs.shape[:2] + (N + pad,), NAN, np.float32)
    xp[:, :N], rp[:, :, :N] = x, refs
    return xp, rp


_want = {}


def want_of(N, R, win):
    """The checker's figures of the standard batch, computed once per (N, R, window)."""
    key = (N, R, win)
    if key not in _want:
        x, refs = batch(N, R)
        _want[key] = tsr.reference(x, FIRST, refs, win)
    return _want[key]


def scores_of(torch, N, x, refs, first=FIRST, win=None):
    """Plan.trace_scores on the [:, :N] views; (scores, energy) as numpy and the stats."""
    pl = plan_of(N)
    xd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(refs).cuda()
    sc, en = pl.trace_scores(xd[:, :N], first, rd[..., :N], window=win, energy=True)
    return sc.cpu().numpy(), en.cpu().numpy(), pl.trace_scores_stats()


def test_scalar_route(lib, torch):
    N = 1501
    x, refs = batch(N)
    sc, en, st = scores_of(torch, N, x, refs)
    assert st == dict(vec=0, segments=1, rounds=1, empty=1), st
    assert sc.shape == (2, 3, 71) and en.shape == (71,)
    tsr.check(sc, en, want_of(N, 2, None), "scalar route")


@pytest.mark.parametrize("win", [(0, 0), (3, 2045), (1024, 1025), (4, 8)], ids=["full", "3-2045", "1024-1025", "4-8"])
@pytest.mark.parametrize("pad", [0, 4], ids=["ld2048", "ld2052"])
def test_vector_route(lib, torch, pad, win):
    N = 2048
    x, refs = batch(N, pad=pad)
    if pad:
        assert np.isnan(x[:, N:]).all() and np.isnan(refs[:, :, N:]).all()
    sc, en, st = scores_of(torch, N, x, refs, win=win)
    assert st == dict(vec=1, segments=1, rounds=1, empty=1), st
    tsr.check(sc, en, want_of(N, 2, win), f"vector route, ld {N + pad}, window {win}")
    if pad:  # the NaN pad columns of traces and references change nothing
        sc0, en0, _ = scores_of(torch, N, *batch(N), win=win)
        assert np.array_equal(sc, sc0, equal_nan=True) and np.array_equal(en, en0)


def test_unaligned_base_takes_the_scalar_route(lib, torch):
    """max % 4 == 0 but the trace rows start 4 bytes off a 16-byte boundary (ld = 2049 views of a flat buffer): scalar loads."""
    N = 2048
    x, refs = batch(N)
    flat = torch.full((x.shape[0] * (N + 1) + 1,), NAN, dtype=torch.float32, device="cuda")
    xv = flat[1:].view(x.shape[0], N + 1)[:, :N]
    xv.copy_(torch.from_numpy(x))
    pl = plan_of(N)
    sc, en = pl.trace_scores(xv, FIRST, torch.from_numpy(refs).cuda(), energy=True)
    assert pl.trace_scores_stats()["vec"] == 0
    tsr.check(sc.cpu().numpy(), en.cpu().numpy(), want_of(N, 2, None), "unaligned base")


@pytest.mark.parametrize("N,vec", [(8193, 0), (8196, 1)], ids=["scalar8193", "vector8196"])
def test_three_column_segments(lib, torch, N, vec):
    """2 * 4096 + 1 samples: the smallest length with three column segments, the last one ragged (one sample); 8196 the same on the vector
    route (one 16-byte load).  Also with a window that leaves a scalar head and tail around three segments."""
    x, refs = batch(N)
    sc, en, st = scores_of(torch, N, x, refs)
    assert st["segments"] >= 3 and st["vec"] == vec, st
    tsr.check(sc, en, want_of(N, 2, None), f"three segments, N {N}")
    if vec:
        win = (1, N - 1)  # head 1 .. 3, body 4 .. 8191 (two segments), tail 8192 .. 8194
        sc, en, st = scores_of(torch, N, x, refs, win=win)
        assert st["segments"] == 2 and st["vec"] == 1, st
        tsr.check(sc, en, want_of(N, 2, win), f"head and tail, N {N}")


def test_zero_energy_and_wide_range(lib, torch):
    N = 2048
    x, refs = batch(N)
    sc, en, st = scores_of(torch, N, x, refs)
    want = want_of(N, 2, None)
    tsr.check(sc, en, want, "zero energy")
    sim, mis, dot = sc[:, 0], sc[:, 1], sc[:, 2]
    dead = 9 - int(FIRST[0])  # the all-zero trace: NaN against every reference, and exactly there -- but for the all-zero reference (0, 1)
    assert np.isnan(sim[:, dead]).all() and np.isnan(sim[1, :SIZES[0]]).all()
    assert not np.isnan(sim[0, np.arange(71) != dead]).any() and not np.isnan(sim[1, SIZES[0]:]).any()
    assert en[dead] == 0 and (dot[:, dead] == 0).all() and (dot[1, :SIZES[0]] == 0).all()
    # the misfit of a dead trace is its reference's energy, the misfit against a dead reference the trace's energy: inside the bound of a sum of squares
    rr = (refs[0, 0].astype(tsr.LD) ** 2).sum()
    assert abs(tsr.LD(mis[0, dead]) - rr) <= 1.01 * (N + 3) * tsr.U * rr and mis[1, dead] == 0
    assert (np.abs(mis[1, :SIZES[0]].astype(tsr.LD) - want["energy"][:SIZES[0]]) <= 1.01 * (N + 3) * tsr.U * want["energy"][:SIZES[0]]).all()
    # the float range: 1e30 and 1e-30 stay finite and accurate in the FP64 sums
    for t, lo, hi in ((11 - int(FIRST[0]), 1e57, 1e64), (12 - int(FIRST[0]), 1e-63, 1e-56)):
        assert lo < en[t] < hi and np.isfinite(sc[0, :, t]).all() and np.isfinite(sc[1, 1:, t]).all() and abs(sim[0, t]) <= 1, (t, en[t])  # (reference (0, 1) is dead: sim NaN)


@pytest.mark.parametrize("N", [1501, 2048], ids=["scalar", "vector"])
def test_reference_counts(lib, torch, N):
    """R = 1, 3, 4 against the checker; plane k of an R-reference call is bit-equal to the R = 1 call on reference k."""
    for R in (1, 3, 4):
        x, refs = batch(N, R)
        sc, en, st = scores_of(torch, N, x, refs)
        assert sc.shape == (R, 3, 71)
        tsr.check(sc, en, want_of(N, R, None), f"R = {R}, N {N}")
        for k in range(R):
            one, en1, _ = scores_of(torch, N, x, np.ascontiguousarray(refs[:, k:k + 1]))
            assert np.array_equal(one[0], sc[k], equal_nan=True) and np.array_equal(en1, en), (R, k)
        if R == 1:  # [B][N] references are R = 1
            pl = plan_of(N)
            two = pl.trace_scores(torch.from_numpy(x).cuda(), FIRST, torch.from_numpy(refs[:, 0]).cuda())
            assert np.array_equal(two.cpu().numpy(), sc, equal_nan=True)


@pytest.mark.parametrize("N", [1501, 2048, 8196], ids=["scalar", "vector", "segments"])
def test_loop_equivalence_and_repeatability(lib, torch, N):
    x, refs = batch(N)
    sc, en, _ = scores_of(torch, N, x, refs, win=(5, N - 2))
    again, en2, _ = scores_of(torch, N, x, refs, win=(5, N - 2))
    assert np.array_equal(sc, again, equal_nan=True) and np.array_equal(en, en2)
    for b in range(len(SIZES)):
        one, en1, _ = scores_of(torch, N, x, refs[b:b + 1], first=FIRST[b:b + 2], win=(5, N - 2))
        c = slice(int(FIRST[b] - FIRST[0]), int(FIRST[b + 1] - FIRST[0]))
        assert one.shape == (2, 3, SIZES[b])
        assert np.array_equal(one, sc[:, :, c], equal_nan=True) and np.array_equal(en1, en[c]), b


def raw_call(lib, torch, pl, x, first, refs, R, ldr, win, scores, energy, ld=None, traces=True):
    f = np.ascontiguousarray(first, dtype=np.uint64)
    return lib.tspws_hip_trace_scores(pl.h, x.data_ptr() if traces else None, x.stride(0) if ld is None else ld, f.ctypes.data, f.size - 1, refs.data_ptr(), ldr, R,
                                      win[0], win[1], scores.data_ptr(), energy.data_ptr() if energy is not None else None,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_guard_cells_early_returns_and_refusals(lib, torch):
    N, G = 2048, 64
    pl = plan_of(N)
    x, refs = batch(N)
    xd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(refs).cuda()
    T = int(FIRST[-1] - FIRST[0])
    sbuf = torch.full((G + 2 * 3 * T + G,), -3.0, dtype=torch.float64, device="cuda")
    ebuf = torch.full((G + T + G,), -4.0, dtype=torch.float64, device="cuda")
    rc = raw_call(lib, torch, pl, xd, FIRST, rd, 2, N, (0, 0), sbuf[G:], ebuf[G:])
    assert rc == 0, lib.tspws_hip_last_error()
    s, e = sbuf.cpu().numpy(), ebuf.cpu().numpy()
    assert (s[:G] == -3.0).all() and (s[-G:] == -3.0).all() and (e[:G] == -4.0).all() and (e[-G:] == -4.0).all()
    ref_sc, ref_en, _ = scores_of(torch, N, x, refs)
    assert np.array_equal(s[G:-G].reshape(2, 3, T), ref_sc, equal_nan=True) and np.array_equal(e[G:-G], ref_en)
    # without an energy output
    sbuf.fill_(-3.0)
    assert raw_call(lib, torch, pl, xd, FIRST, rd, 2, N, (0, 0), sbuf[G:], None) == 0
    assert np.array_equal(sbuf.cpu().numpy()[G:-G].reshape(2, 3, T), ref_sc, equal_nan=True)
    # B = 0 and T = 0 with a plan: 0, nothing written
    sbuf.fill_(-3.0)
    ebuf.fill_(-4.0)
    f = np.array([5], np.uint64)
    assert lib.tspws_hip_trace_scores(pl.h, xd.data_ptr(), N, f.ctypes.data, 0, rd.data_ptr(), N, 2, 0, 0, sbuf.data_ptr(), ebuf.data_ptr(), None) == 0
    assert raw_call(lib, torch, pl, xd, [5, 5, 5], rd, 2, N, (0, 0), sbuf, ebuf) == 0
    assert raw_call(lib, torch, pl, xd, [5, 5, 5], rd, 2, N, (0, 0), sbuf, ebuf, traces=False) == 0  # (no traces needed without columns)
    # what needs the plan's trace length
    for kw, msg in ((dict(ld=N - 1), b"trace_scores: row stride below"), (dict(ldr=N - 1), b"trace_scores: reference row stride below"),
                    (dict(win=(0, N + 1)), b"trace_scores: a lag window past"), (dict(win=(N, 0)), b"trace_scores: an empty lag window"),
                    (dict(traces=False), b"trace_scores: NULL traces")):
        args = dict(ld=None, ldr=N, win=(0, 0), traces=True)
        args.update(kw)
        rc = raw_call(lib, torch, pl, xd, FIRST, rd, 2, args["ldr"], args["win"], sbuf, ebuf, ld=args["ld"], traces=args["traces"])
        assert rc == -1 and msg in lib.tspws_hip_last_error(), (kw, lib.tspws_hip_last_error())
    torch.cuda.synchronize()
    assert bool((sbuf == -3.0).all()) and bool((ebuf == -4.0).all())
    # the binding refuses what the C ABI cannot see
    with pytest.raises(tspws.TspwsError):
        pl.trace_scores(xd, FIRST, rd[:2])
    with pytest.raises(tspws.TspwsError):
        pl.trace_scores(xd, FIRST, rd.double())


def test_small_budget_takes_rounds_bit_identically(lib, torch, tmp_path):
    """The 16.9 MB of partial sums under TSPWS_PART_MB=16 in a child process (2 rounds) against the one-round scores of this process."""
    one, en, st = tsc.run(torch)
    assert st == dict(vec=0, segments=1, rounds=1, empty=0), st
    assert np.isfinite(one).all() and np.isfinite(en).all()
    # a trace against itself: sim 1 and misfit 0 (rows 0 and 1 of either ensemble are its references)
    assert abs(one[0, 0, 0] - 1) <= (2 * tsc.N + 8) * tsr.U and one[0, 1, 0] == 0 and one[1, 1, tsc.M + 1] == 0
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "trace_scores_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "SCORES_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert int(small["rounds"]) >= 2 and int(small["vec"]) == 0 and int(small["segments"]) == 1
    assert np.array_equal(small["scores"], one) and np.array_equal(small["energy"], en)
