"""The band-limited batched stack (tspws_hip_stack_batch_bands, Plan.stack_batch_bands) on the GPU: the batch of tests/batch_engine.batch --
ensembles of 1, 3, 5, 8, 0 and 67 traces, first0 = 2, pad = 5 -- on three frames in three modes, every ls / ts / ls_env / ts_env row within the
project's parity figure (abi.relerr <= 2e-6) of the definition applied literally in numpy (tests/band_batch_ref.py); empty ensembles and
bands exactly zero; [0, S) against Plan.stack_batch; envelope=False bit for bit; B = 1; a small scratch budget in a child process; one long
frame whose bands cut an octave.  The worst ratios go to TSPWS_BAND_REPORT when it is set."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import band_batch_ref as bbr

pytestmark = pytest.mark.gpu

TOL32 = 2e-6
SIZES = [1, 3, 5, 8, 0, 67]
tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))

FRAMES = {"morlet-2048": (dict(), 2048), "morlet-1501": (dict(), 1501), "mexhat-2048": (dict(type=-3), 2048)}
# biased wu = 2; unbiased; Kmax = 4 unbiased: the ensembles with M_b >= 4 are two-stage, the rest single-stage
MODES = {"biased": dict(), "unbiased": dict(unbiased=1), "kmax4-unbiased": dict(unbiased=1, Kmax=4)}


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


def report(line):
    print(line, flush=True)
    path = os.environ.get("TSPWS_BAND_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def make_batch(torch, kw, sizes, N, seed, first0=2, pad=5):
    """tests/batch_engine.batch's batch: (plan, params, traces numpy, offsets, padded device array)."""
    p = abi.default_params(**kw)
    pl = tspws.Plan(tspws.resolve(p, N), N)
    first = np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)
    X = abi.synth_traces(int(first[-1]), N, seed=seed)
    buf = torch.zeros((X.shape[0], N + pad), dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    return pl, abi.resolve(p, N), X, first, buf


def frequency_bands(pl):
    """R = 3 bands with shared edges from bands_from_frequencies -- the edges are geometric means of neighbouring centre frequencies, between two
    voices of an octave where the frame has more than one -- plus [0, S), plus an empty one."""
    S, V = pl.S, pl.info.V
    _, fc = tspws.bands_from_frequencies(pl, 1.0, [1.0, 2.0])
    k1, k2 = (k + 1 if V > 1 and k % V == 0 else k for k in (S // 3, 2 * S // 3))
    assert 0 < k1 < k2 < S
    edges = [float(fc[-1]) * 0.5, float(np.sqrt(fc[k2] * fc[k2 - 1])), float(np.sqrt(fc[k1] * fc[k1 - 1])), float(fc[0]) * 2]
    bands, _ = tspws.bands_from_frequencies(pl, 1.0, edges)
    assert bands.tolist() == [[k2, S], [k1, k2], [0, k1]], (bands, k1, k2, S)   # lowest band first: they partition the scales
    return [tuple(int(v) for v in b) for b in bands] + [(0, S), (2, 2)]


def worst_rows(got, want, what):
    """max over the rows of abi.relerr(row, expected row); zero expected rows must be exactly zero."""
    w = 0.0
    for idx in np.ndindex(want.shape[:-1]):
        if not want[idx].any():
            assert not got[idx].any(), (what, idx, "a zero row")
        else:
            e = abi.relerr(got[idx], want[idx])
            assert e <= TOL32, (what, idx, e)
            w = max(w, e)
    return w


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_batch_bands(lib, torch, frame, mode):
    kw, N = FRAMES[frame]
    pl, p, X, first, buf = make_batch(torch, dict(kw, **MODES[mode]), SIZES, N, seed=N + len(mode))
    bands = frequency_bands(pl)
    R = len(bands)
    ls, ts, ls_env, ts_env = (t.cpu().numpy() for t in pl.stack_batch_bands(buf[:, :N], first, bands, envelope=True))
    st = pl.stack_batch_bands_stats()
    want = bbr.expected(p, X, first, bands)
    w = {k: worst_rows(g, e, k) for k, g, e in zip(("ls", "ts", "ls_env", "ts_env"), (ls, ts, ls_env, ts_env), want)}
    # empty ensemble, empty band: exactly zero (and written: the outputs held NaN)
    for o in (ls, ts, ls_env, ts_env):
        assert not o[SIZES.index(0)].any() and not o[:, R - 1].any() and np.isfinite(o).all()
    union = len({s for a, e in bands for s in range(a, e)})
    assert st["scales"] == union == pl.S and st["quadrature"] == 1 and st["empty"] == 1 and st["finish_batches"] >= 1, st
    assert st["single_pass"] + st["two_stage_pass"] + st["looped"] == 5, st
    if mode == "kmax4-unbiased":
        assert st["two_stage_pass"] == 3 and st["looped"] == 2, st     # M_b = 5, 8, 67 share the two-stage pass
    # [0, S) against the plain batched stack
    l0, t0 = (t.cpu().numpy() for t in pl.stack_batch(buf[:, :N], first))
    assert {k: pl.batch_stats()[k] for k in ("single_pass", "two_stage_pass", "looped", "empty")} == \
        {k: st[k] for k in ("single_pass", "two_stage_pass", "looped", "empty")}
    w["ls [0, S) / stack_batch"] = worst_rows(ls[:, R - 2], l0, "ls [0, S)")
    w["ts [0, S) / stack_batch"] = worst_rows(ts[:, R - 2], t0, "ts [0, S)")
    # without the envelopes: the same bits, no quadrature work
    l1, t1 = (t.cpu().numpy() for t in pl.stack_batch_bands(buf[:, :N], first, bands))
    assert pl.stack_batch_bands_stats()["quadrature"] == 0
    assert l1.tobytes() == ls.tobytes() and t1.tobytes() == ts.tobytes()
    # B = 1: the single-ensemble call (the largest ensemble and a small one)
    for b in (5, 1):
        one = [t.cpu().numpy() for t in pl.stack_batch_bands(buf[:, :N], first[b: b + 2], bands, envelope=True)]
        for k, g, e in zip(("ls", "ts", "ls_env", "ts_env"), one, (ls, ts, ls_env, ts_env)):
            w[f"{k} B = 1"] = max(w.get(f"{k} B = 1", 0.0), worst_rows(g[0], e[b], f"{k} B = 1, ensemble {b}"))
    report(f"BAND_BATCH {frame} {mode}: bands {bands} | " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f" | {st}")


def test_shared_single_pass(lib, torch):
    """Ensembles whose total takes the many-trace path: the band finish behind the shared single-stage pass (the batch above is below it)."""
    N = 2048
    pl, p, X, first, buf = make_batch(torch, dict(unbiased=1), [130, 0, 70, 64], N, seed=4)
    bands = frequency_bands(pl)
    got = [t.cpu().numpy() for t in pl.stack_batch_bands(buf[:, :N], first, bands, envelope=True)]
    st = pl.stack_batch_bands_stats()
    assert st["single_pass"] == 3 and st["looped"] == 0 and st["empty"] == 1 and st["finish_batches"] == st["rounds"] == 1, st
    want = bbr.expected(p, X, first, bands)
    w = {k: worst_rows(g, e, k) for k, g, e in zip(("ls", "ts", "ls_env", "ts_env"), got, want)}
    report(f"BAND_BATCH shared single-stage pass N = {N}: bands {bands} | " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f" | {st}")


def test_small_budget_child():
    """TSPWS_PART_MB=16 in a child process (the library reads it once): more than one finish batch, by _stats; the same figure."""
    env = dict(os.environ, TSPWS_PART_MB="16")
    out = subprocess.run([sys.executable, os.path.join(HERE, "band_batch_child.py")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("BAND_BATCH_CHILD")]
    assert line, out.stdout[-3000:]
    report(line[-1])


def test_long_frame_cut_octave(lib, torch):
    """2 ensembles of 3 traces at N = 32768 (the wave-uniform scales with D > 64, whose octave items the plain inverse does not split): bands
    that cut octaves between voices."""
    N = 32768
    pl, p, X, first, buf = make_batch(torch, dict(), [3, 3], N, seed=9, first0=0, pad=0)
    S, V = pl.S, pl.info.V
    assert pl.inverse_info()["per_scale"] == 0 and V == 4
    bands = [(0, S - 2 * V - 2), (S - 2 * V - 2, S - V - 1), (S - V - 1, S), (S - 3, S - 1)]
    got = [t.cpu().numpy() for t in pl.stack_batch_bands(buf, first, bands, envelope=True)]
    want = bbr.expected(p, X, first, bands)
    w = {k: worst_rows(g, e, k) for k, g, e in zip(("ls", "ts", "ls_env", "ts_env"), got, want)}
    # the first three bands partition the scales: their rows add up to the plain stack, to the figure
    l0, t0 = (t.cpu().numpy() for t in pl.stack_batch(buf, first))
    for b in range(2):
        assert abi.relerr(got[0][b, :3].astype(np.float64).sum(axis=0), l0[b]) <= TOL32
        assert abi.relerr(got[1][b, :3].astype(np.float64).sum(axis=0), t0[b]) <= TOL32
    report(f"BAND_BATCH long N = {N}: bands {bands} | " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f" | {pl.stack_batch_bands_stats()}")


def test_arguments(lib, torch):
    N = 2048
    pl, p, X, first, buf = make_batch(torch, dict(), [3, 2], N, seed=1)
    S = pl.S
    for bad in ([(0, S + 1)], [(2, 1)], [(0, 1)] * 1025):
        with pytest.raises(tspws.TspwsError):
            pl.stack_batch_bands(buf[:, :N], first, bad)
    with pytest.raises(tspws.TspwsError):
        pl.stack_batch_bands(buf[:, :N], [0, 3, 2], [(0, 1)])
    # the C entry point: refused before any device work, outputs untouched
    out = torch.full((2, 1, N), 7.0, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = np.ascontiguousarray(first, dtype=np.uint64)
    bt = tspws.band_table([(0, S + 1)])
    ok = tspws.band_table([(0, S)])
    args = (pl.h, C.byref(pl.params), buf.data_ptr(), N + 5, f.ctypes.data, 2)
    assert lib.tspws_hip_stack_batch_bands(*args, bt.ctypes.data, 1, out.data_ptr(), out.data_ptr(), None, None, stream) == -1
    assert b"stack_batch_bands: a band ends behind the last scale" in lib.tspws_hip_last_error()
    assert lib.tspws_hip_stack_batch_bands(*args, ok.ctypes.data, 1, out.data_ptr(), out.data_ptr(), out.data_ptr(), None, stream) == -1
    assert lib.tspws_hip_stack_batch_bands(*args, ok.ctypes.data, 1, None, out.data_ptr(), None, None, stream) == -1
    assert lib.tspws_hip_stack_batch_bands(pl.h, C.byref(pl.params), buf.data_ptr(), N - 1, f.ctypes.data, 2, ok.ctypes.data, 1, out.data_ptr(), out.data_ptr(),
                                           None, None, stream) == -1
    # R = 0 / B = 0: nothing to do
    assert lib.tspws_hip_stack_batch_bands(*args, ok.ctypes.data, 0, out.data_ptr(), out.data_ptr(), None, None, stream) == 0
    assert lib.tspws_hip_stack_batch_bands(pl.h, C.byref(pl.params), buf.data_ptr(), N + 5, f.ctypes.data, 0, ok.ctypes.data, 1, None, None, None, None, stream) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ls, ts = pl.stack_batch_bands(buf[:, :N], first, [])
    assert tuple(ls.shape) == (2, 0, N)
