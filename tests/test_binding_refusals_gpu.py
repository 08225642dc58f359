"""The binding's own argument checks (ts-pws_amd/__init__.py), method by method: every row of ROWS passes ONE wrong argument to a Plan
method and names the TspwsError text it must raise -- the texts as the binding gave them before its methods shared their checks.  (Four of
the copies did not ask whether an output is a tensor at all: a list given as `ls` / `ls_out` to stack_single, stack_batch, jackknife_single
and jackknife_finish ended in an AttributeError.  Those rows hold the text the sibling methods gave.)  Every wrong argument is one the Python
layer refuses before the C call: no row reaches a kernel.  test_good_arguments shows that the shared checks refuse nothing that is right:
given outputs come back as the very objects, views of a wider base and strided counts pass, every *_stats() has its names.

One plan (default parameters, N = 512), 7 synthetic traces, first = [0, 3, 3, 7] (the middle ensemble empty), M = C = 3; a second plan with
Kmax = 2 for the two-stage calls."""
import importlib
import types

import numpy as np
import pytest

import abi

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N, F = 512, [0, 3, 3, 7]


@pytest.fixture(scope="module")
def env():
    import torch
    assert tspws.load().tspws_hip_device_count() > 0 and torch.cuda.is_available(), "no MI355X visible (there is no CPU fallback)"
    e = types.SimpleNamespace(t=torch)
    e.pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    e.pl2 = tspws.Plan(tspws.resolve(abi.default_params(Kmax=2), N), N)
    e.X = tspws.synth(7, N, seed=3)
    e.f32 = lambda *shape, **kw: torch.zeros(shape, dtype=torch.float32, device=kw.get("device", "cuda"))  # noqa: E731
    e.f64 = lambda *shape, **kw: torch.zeros(shape, dtype=torch.float64, device=kw.get("device", "cuda"))  # noqa: E731
    e.sel = np.ones((3, 7), np.int8)
    e.sel[[0, 1, 2, 0], [0, 1, 5, 6]] = 0
    e.masks = np.zeros((3, 7), np.int8)  # three ones a row: K = ceil(7 * 0.4)
    e.masks[0, :3] = e.masks[1, 2:5] = e.masks[2, 4:] = 1
    e.cnt = np.array([[1, 2, 0, 0, 1, 3, 0], [0, 0, 3, 2, 2, 0, 0], [1, 1, 1, 1, 1, 1, 1]], np.uint8)
    e.w = np.array([[1.0, 0.5, 0.0, 2.0, 0.25, 0.0, 1.0], [0.0] * 7, [1.0] * 7])
    e.rows = torch.sin(torch.arange(3 * 3 * N, dtype=torch.float32, device="cuda") * 0.05).reshape(3, 3, N)
    e.ref = e.rows[:, 0].contiguous()
    e.eps = tspws.stretch_grid(0.01, 5)
    e.win = ((10, 200),)
    e.Y = np.zeros((2, e.pl.ncoef), np.complex128)
    yield e
    e.pl.close()
    e.pl2.close()


# (id, call on the environment, the message)
ROWS = [
    # ---- first: not integer / decreasing / past the rows
    ("stack_batch-first-float", lambda e: e.pl.stack_batch(e.X, [0.0, 3.0, 3.0, 7.0]),
     "first must be a 1-D integer array of B + 1 ensemble offsets"),
    ("stack_batch_bands-first-float", lambda e: e.pl.stack_batch_bands(e.X, np.array([0.0, 3.0, 7.0]), [(0, 2)]),
     "first must be a 1-D integer array of B + 1 ensemble offsets"),
    ("jackknife_batch-first-2d", lambda e: e.pl.jackknife_batch(e.X, [[0, 3], [3, 7]], e.sel),
     "first must be a 1-D integer array of B + 1 ensemble offsets"),
    ("convergence_batch-first-empty", lambda e: e.pl.convergence_batch(e.X, []),
     "first must be a 1-D integer array of B + 1 ensemble offsets"),
    ("subsample_batch-first-decreasing", lambda e: e.pl.subsample_batch(e.X, [0, 3, 2, 7], e.masks),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("bootstrap_batch-first-decreasing", lambda e: e.pl.bootstrap_batch(e.X, [0, 3, 2, 7], e.cnt),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("weighted_stack_batch-first-negative", lambda e: e.pl.weighted_stack_batch(e.X, [-1, 3, 3, 6], e.w),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("jackknife_batch_two_stage-first-decreasing", lambda e: e.pl2.jackknife_batch_two_stage(e.X, [0, 3, 2, 7], e.sel),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("stack_batch-first-past", lambda e: e.pl.stack_batch(e.X, [0, 3, 3, 8]),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("stack_batch_bands-first-past", lambda e: e.pl.stack_batch_bands(e.X, [0, 3, 3, 8], [(0, 2)]),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("trace_scores-first-past", lambda e: e.pl.trace_scores(e.X, [0, 3, 3, 8], e.ref),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("selective_stack_batch-first-past", lambda e: e.pl.selective_stack_batch(e.X, [0, 3, 3, 8]),
     "first must be non-decreasing offsets into the 7 trace rows"),
    ("convergence_batch-first-past", lambda e: e.pl.convergence_batch(e.X, [0, 3, 3, 8]),
     "first must be non-decreasing offsets into the 7 trace rows"),
    # ---- an output of the wrong dtype
    ("stack_single-ls-dtype", lambda e: e.pl.stack_single(e.X, ls=e.f64(N)),
     "ls must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("stack_batch-ls-dtype", lambda e: e.pl.stack_batch(e.X, F, ls=e.f64(3, N)),
     "ls must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_batch-ls_out-dtype", lambda e: e.pl.jackknife_batch(e.X, F, e.sel, ls_out=e.f64(3, 3, N)),
     "ls_out must be a contiguous float32 [3, 3, 512] tensor on cuda:0"),
    ("subsample_sel-ts_out-dtype", lambda e: e.pl.subsample_sel(e.X, e.masks, 0.4, ts_out=e.f64(3, N)),
     "ts_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("replica_bands-out-dtype", lambda e: e.pl.replica_bands(e.rows, [0.1, 0.9], out=e.f64(3, 2, N)),
     "out must be a contiguous float32 [3][2][512] tensor on cuda:0"),
    ("stretch_rows-fit-dtype", lambda e: e.pl.stretch_rows(e.rows, e.ref, 256.0, e.eps, e.win, out=e.f32(3, 3, 1, 4)),
     "out: fit must be a contiguous float64 tensor of >= 36 values on cuda:0"),
    ("convergence-ref_ts-dtype", lambda e: e.pl.convergence(e.X, e.f64(N), e.f32(N)),
     "ref_ts must be a contiguous float32 [1][512] tensor on cuda:0"),
    # ---- an output of the wrong shape
    ("stack_finish-ls-short", lambda e: e.pl.stack_finish(7, e.f32(N - 1), e.f32(N)),
     "ls must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("jackknife_single-ls_out-shape", lambda e: e.pl.jackknife_single(e.X, e.sel, ls_out=e.f32(2, N)),
     "ls_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_batch-ls-shape", lambda e: e.pl.jackknife_batch(e.X, F, e.sel, ls=e.f32(2, N)),
     "ls must be a contiguous float32 [3, 512] tensor on cuda:0"),
    ("jackknife_batch_two_stage-ts_out-shape", lambda e: e.pl2.jackknife_batch_two_stage(e.X, F, e.sel, ts_out=e.f32(3, 3, N + 1)),
     "ts_out must be a contiguous float32 [3, 3, 512] tensor on cuda:0"),
    ("subsample_batch-ts_out-shape", lambda e: e.pl.subsample_batch(e.X, F, e.masks, ts_out=e.f32(3, 3, N + 1)),
     "ts_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    ("convergence_batch-ref_ls-shape", lambda e: e.pl.convergence_batch(e.X, F, e.f32(3, N), e.f32(2, N)),
     "ref_ls must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("stretch_rows-cc-short", lambda e: e.pl.stretch_rows(e.rows, e.ref, 256.0, e.eps, e.win, cc=True, out=(e.f64(44), e.f64(36))),
     "out: cc must be a contiguous float64 tensor of >= 45 values on cuda:0"),
    # ---- a non-contiguous output
    ("stack_finish_tail-ts-strided", lambda e: e.pl.stack_finish_tail(7, e.f32(N), e.f32(2 * N)[::2]),
     "ts must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("bootstrap_batch-ls_out-strided", lambda e: e.pl.bootstrap_batch(e.X, F, e.cnt, ls_out=e.f32(3, 3, N + 8)[:, :, :N]),
     "ls_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    ("weighted_stack_batch-ts_out-strided", lambda e: e.pl.weighted_stack_batch(e.X, F, e.w, ts_out=e.f32(3, N, 3).permute(0, 2, 1)),
     "ts_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    ("replica_bands-out-strided", lambda e: e.pl.replica_bands(e.rows, [0.5], out=e.f32(3, 1, N + 8)[:, :, :N]),
     "out must be a contiguous float32 [3][1][512] tensor on cuda:0"),
    # ---- an output on the CPU
    ("epilogue-ls-cpu", lambda e: e.pl.epilogue(e.f64(2 * N), 7, e.f32(N, device="cpu"), e.f32(N)),
     "ls must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("stack_batch-ts-cpu", lambda e: e.pl.stack_batch(e.X, F, ts=e.f32(3, N, device="cpu")),
     "ts must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_finish-ts_out-cpu", lambda e: e.pl2.jackknife_finish(7, e.sel, 0, 3, e.f32(3, N), e.f32(3, N, device="cpu"), np.zeros(3, np.uint32)),
     "ts_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("weighted_stack_batch-ls_out-cpu", lambda e: e.pl.weighted_stack_batch(e.X, F, e.w, ls_out=e.f32(3, 3, N, device="cpu")),
     "ls_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    ("stretch_rows-fit-cpu", lambda e: e.pl.stretch_rows(e.rows, e.ref, 256.0, e.eps, e.win, out=e.f64(36, device="cpu")),
     "out: fit must be a contiguous float64 tensor of >= 36 values on cuda:0"),
    ("convergence_batch-ref_ts-cpu", lambda e: e.pl.convergence_batch(e.X, F, e.f32(3, N, device="cpu"), e.f32(3, N)),
     "ref_ts must be a contiguous float32 [3][512] tensor on cuda:0"),
    # ---- a numpy array or a list given as an output
    ("stack_single-ls-numpy", lambda e: e.pl.stack_single(e.X, ls=np.zeros(N, np.float32)),
     "ls must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("stack_single-ls-list", lambda e: e.pl.stack_single(e.X, ls=[0.0] * N),
     "ls must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("stack_batch-ts-list", lambda e: e.pl.stack_batch(e.X, F, ts=[[0.0] * N] * 3),
     "ts must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_single-ts_out-list", lambda e: e.pl.jackknife_single(e.X, e.sel, ts_out=[[0.0] * N] * 3),
     "ts_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_finish-ls_out-list", lambda e: e.pl2.jackknife_finish(7, e.sel, 0, 3, [[0.0] * N] * 3, e.f32(3, N), np.zeros(3, np.uint32)),
     "ls_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("stack_jackknife-ts-numpy", lambda e: e.pl2.stack_jackknife(e.X, e.sel, ts=np.zeros(N, np.float32)),
     "ts must be a contiguous float32 tensor of >= 512 samples on cuda:0"),
    ("stack_batch-ls-numpy", lambda e: e.pl.stack_batch(e.X, F, ls=np.zeros((3, N), np.float32)),
     "ls must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_single-ls_out-numpy", lambda e: e.pl.jackknife_single(e.X, e.sel, ls_out=np.zeros((3, N), np.float32)),
     "ls_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("jackknife_finish-ls_out-numpy", lambda e: e.pl2.jackknife_finish(7, e.sel, 0, 3, np.zeros((3, N), np.float32), e.f32(3, N), np.zeros(3, np.uint32)),
     "ls_out must be a contiguous float32 [3][512] tensor on cuda:0"),
    ("subsample_batch-ls_out-numpy", lambda e: e.pl.subsample_batch(e.X, F, e.masks, ls_out=np.zeros((3, 3, N), np.float32)),
     "ls_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    ("bootstrap_batch-ts_out-numpy", lambda e: e.pl.bootstrap_batch(e.X, F, e.cnt, ts_out=np.zeros((3, 3, N), np.float32)),
     "ts_out must be a contiguous float32 [3][3][512] tensor on cuda:0"),
    # ---- mtr_out / mtr of the wrong dtype
    ("jackknife_single-mtr_out-dtype", lambda e: e.pl.jackknife_single(e.X, e.sel, mtr_out=np.zeros(3, np.int32)),
     "mtr_out must be a contiguous uint32 numpy array of 3 entries"),
    ("jackknife_finish-mtr_out-dtype", lambda e: e.pl2.jackknife_finish(7, e.sel, 0, 3, e.f32(3, N), e.f32(3, N), np.zeros(3, np.int64)),
     "mtr_out must be a contiguous uint32 numpy array of 3 entries"),
    ("subsample_batch-mtr_out-dtype", lambda e: e.pl.subsample_batch(e.X, F, e.masks, mtr_out=np.zeros((3, 3), np.int32)),
     "mtr_out must be a contiguous uint32 numpy array [3][3]"),
    ("bootstrap_batch-mtr_out-list", lambda e: e.pl.bootstrap_batch(e.X, F, e.cnt, mtr_out=[[0] * 3] * 3),
     "mtr_out must be a contiguous uint32 numpy array [3][3]"),
    ("replica_bands-mtr-dtype", lambda e: e.pl.replica_bands(e.rows, [0.5], mtr=np.ones((3, 3), np.int32)),
     "mtr must be None or a uint32 numpy array [3][3]"),
    # ---- mtr_out / mtr of the wrong shape
    ("jackknife_single-mtr_out-shape", lambda e: e.pl.jackknife_single(e.X, e.sel, mtr_out=np.zeros(4, np.uint32)),
     "mtr_out must be a contiguous uint32 numpy array of 3 entries"),
    ("jackknife_batch-mtr_out-shape", lambda e: e.pl.jackknife_batch(e.X, F, e.sel, mtr_out=np.zeros((3, 4), np.uint32)),
     "mtr_out must be a contiguous uint32 numpy array [3][3]"),
    ("jackknife_batch_two_stage-mtr_out-strided", lambda e: e.pl2.jackknife_batch_two_stage(e.X, F, e.sel, mtr_out=np.zeros((3, 6), np.uint32)[:, ::2]),
     "mtr_out must be a contiguous uint32 numpy array [3][3]"),
    ("weighted_stack_batch-mtr_out-shape", lambda e: e.pl.weighted_stack_batch(e.X, F, e.w, mtr_out=np.zeros(9, np.uint32)),
     "mtr_out must be a contiguous uint32 numpy array [3][3]"),
    ("stretch_rows-mtr-shape", lambda e: e.pl.stretch_rows(e.rows, e.ref, 256.0, e.eps, e.win, mtr=np.ones((3, 2), np.uint32)),
     "mtr must be None or a uint32 numpy array [3][3]"),
    # ---- a float selection
    ("jackknife_single-sel-float", lambda e: e.pl.jackknife_single(e.X, e.sel.astype(np.float64)),
     "selection must be a 2-D int8 / uint8 / bool numpy array [C][mtr]"),
    ("jackknife_batch-sel-float", lambda e: e.pl.jackknife_batch(e.X, F, e.sel.astype(np.float32)),
     "selection must be a 2-D int8 / uint8 / bool numpy array [C][T]"),
    ("jackknife_batch_two_stage-sel-list", lambda e: e.pl2.jackknife_batch_two_stage(e.X, F, e.sel.tolist()),
     "selection must be a 2-D int8 / uint8 / bool numpy array [C][T]"),
    ("subsample_sel-masks-float", lambda e: e.pl.subsample_sel(e.X, e.masks.astype(np.float64), 0.4),
     "masks must be a 2-D int8 / uint8 / bool numpy array [M][mtr]"),
    ("subsample_batch-masks-float", lambda e: e.pl.subsample_batch(e.X, F, e.masks.astype(np.float64)),
     "masks must be a 2-D int8 / uint8 / bool numpy array [M][T]"),
    ("subsample_batch-masks-1d", lambda e: e.pl.subsample_batch(e.X, F, e.masks[0]),
     "masks must be a 2-D int8 / uint8 / bool numpy array [M][T]"),
    # ---- a selection of the wrong width
    ("jackknife_single-sel-width", lambda e: e.pl.jackknife_single(e.X, e.sel[:, :6]),
     "selection must be [3][7] (replica x trace of the WHOLE ensemble), got (3, 6)"),
    ("jackknife_batch-sel-width", lambda e: e.pl.jackknife_batch(e.X, [1, 3, 3, 7], e.sel),
     "selection must be [3][6] (replica x trace of the WHOLE ensemble), got (3, 7)"),
    ("subsample_sel-masks-width", lambda e: e.pl.subsample_sel(e.X, e.masks[:, :6], 0.4),
     "selection must be [3][7] (replica x trace of the WHOLE ensemble), got (3, 6)"),
    ("subsample_batch-masks-width", lambda e: e.pl.subsample_batch(e.X, F, e.masks[:, 1:]),
     "selection must be [3][7] (replica x trace of the WHOLE ensemble), got (3, 6)"),
    ("stack_jackknife-sel-width", lambda e: e.pl2.stack_jackknife(e.X, e.sel[:, :6]),
     "selection must be [3][7] (replica x trace of the WHOLE ensemble), got (3, 6)"),
    ("jackknife_local-sel-width", lambda e: e.pl2.jackknife_local(e.X, 0, 8, e.sel),
     "selection must be [3][8] (replica x trace of the WHOLE ensemble), got (3, 7)"),
    ("jackknife_finish-sel-width", lambda e: e.pl2.jackknife_finish(8, e.sel, 0, 3, e.f32(3, N), e.f32(3, N), np.zeros(3, np.uint32)),
     "selection must be [3][8] (replica x trace of the WHOLE ensemble), got (3, 7)"),
    # ---- Y with the wrong ncoef / on the CPU
    ("inverse-Y-ncoef", lambda e: e.pl.inverse(e.Y[:, :-1]),
     "Y must be complex128 [nrec >= 1][2016], got complex128 (2, 2015)"),
    ("inverse_bands-Y-ncoef", lambda e: e.pl.inverse_bands(e.t.from_numpy(e.Y[:, 1:]).cuda(), [(0, 2)]),
     "Y must be complex128 [nset >= 1][2016], got torch.complex128 (2, 2015)"),
    ("inverse-Y-cpu", lambda e: e.pl.inverse(e.t.from_numpy(e.Y)),
     "Y must be a contiguous tensor on cuda:0, got cpu"),
    ("inverse_bands-Y-cpu", lambda e: e.pl.inverse_bands(e.t.from_numpy(e.Y), [(0, 2)]),
     "Y must be a contiguous tensor on cuda:0, got cpu"),
    ("inverse-Y-list", lambda e: e.pl.inverse(e.Y.tolist()),
     "Y must be a complex128 numpy array or device tensor"),
    # ---- rows with stride(2) != 1 / a row stride below N
    ("replica_bands-rows-stride2", lambda e: e.pl.replica_bands(e.f32(3, 3, 2 * N)[:, :, ::2], [0.5]),
     "rows must be contiguous along the samples (stride(2) == 1)"),
    ("stretch_rows-rows-stride2", lambda e: e.pl.stretch_rows(e.f32(3, 3, 2 * N)[:, :, ::2], e.ref, 256.0, e.eps, e.win),
     "rows must be contiguous along the samples (stride(2) == 1)"),
    ("trace_scores-refs-stride2", lambda e: e.pl.trace_scores(e.X, F, e.f32(3, 2, 2 * N)[:, :, ::2]),
     "refs must be contiguous along the samples (stride(2) == 1)"),
    ("replica_bands-rows-overlap", lambda e: e.pl.replica_bands(e.f32(3 * 3 * N).as_strided((3, 3, N), (3 * N // 2, N // 2, 1)), [0.5]),
     "overlapping replica rows (row stride < N)"),
    ("stretch_rows-rows-overlap", lambda e: e.pl.stretch_rows(e.f32(3 * 3 * N).as_strided((3, 3, N), (3 * N // 2, N // 2, 1)), e.ref, 256.0, e.eps, e.win),
     "overlapping rows (row stride < N)"),
    ("trace_scores-refs-overlap", lambda e: e.pl.trace_scores(e.X, F, e.f32(3 * 2 * N).as_strided((3, 2, N), (N, N // 2, 1))),
     "overlapping reference rows (row stride < N)"),
    ("replica_bands-rows-base", lambda e: e.pl.replica_bands(e.f32(3, 4, N)[:, :3], [0.5]),
     "rows must be a [B][M][N] view of one [B][M][ld] base (stride(0) == M * stride(1))"),
    ("trace_scores-refs-base", lambda e: e.pl.trace_scores(e.X, F, e.f32(3, 3, N)[:, :2]),
     "refs must be a [B][R][N] view of one [B][R][ld] base (stride(0) == R * stride(1))"),
    ("stretch_rows-rows-cpu", lambda e: e.pl.stretch_rows(e.rows.cpu(), e.ref, 256.0, e.eps, e.win),
     "rows live on cpu, the plan on cuda:0"),
    ("replica_bands-rows-dtype", lambda e: e.pl.replica_bands(e.rows.double(), [0.5]),
     "rows must be a float32 [B][M][512] tensor, got torch.float64 (3, 3, 512)"),
    # ---- x2 of 2 N - 1 values
    ("stack_finish_scales-x2-short", lambda e: e.pl2.stack_finish_scales(7, 0, 1, e.f64(2 * N - 1)),
     "x2 must be a contiguous float64 tensor of 1024 values on cuda:0"),
    ("epilogue-x2-short", lambda e: e.pl.epilogue(e.f64(2 * N - 1), 7, e.f32(N), e.f32(N)),
     "x2 must be a contiguous float64 tensor of 1024 values on cuda:0"),
    ("epilogue-x2-long", lambda e: e.pl.epilogue(e.f64(2 * N + 1), 7, e.f32(N), e.f32(N)),
     "x2 must be a contiguous float64 tensor of 1024 values on cuda:0"),
]


@pytest.mark.parametrize("call,message", [pytest.param(c, m, id=i) for i, c, m in ROWS])
def test_refusals(env, call, message):
    with pytest.raises(tspws.TspwsError) as err:
        call(env)
    assert str(err.value) == message


STATS = {
    "batch_stats": ("single_pass", "two_stage_pass", "looped", "empty", "rounds", "pass_batches"),
    "stack_batch_bands_stats": ("single_pass", "two_stage_pass", "looped", "empty", "rounds", "pass_batches", "finish_batches", "scales", "quadrature"),
    "jackknife_batch_stats": ("shared", "looped", "empty", "rounds", "pass_batches", "classes"),
    "jackknife_batch_two_stage_stats": ("shared", "looped", "empty", "rounds", "tiles", "rows"),
    "subsample_batch_stats": ("single_shared", "two_stage_shared", "looped", "empty", "rounds", "rows"),
    "bootstrap_batch_stats": ("shared", "empty", "rounds", "rows", "max_count"),
    "weighted_stack_batch_stats": ("shared", "empty", "rounds", "rows"),
    "replica_bands_stats": ("lds", "global", "empty", "rounds", "lds_max_rows"),
    "trace_scores_stats": ("vec", "segments", "rounds", "empty"),
    "stretch_rows_stats": ("rounds", "segments", "rows", "left_out", "chunks"),
    "convergence_batch_stats": ("single_steps", "two_stage_steps", "rows", "rounds", "looped", "empty"),
}


def test_good_arguments(env):
    e, torch, pl, pl2 = env, env.t, env.pl, env.pl2
    rows_out = lambda *lead: (e.f32(*lead, N), e.f32(*lead, N), np.full(lead, 99, np.uint32))  # noqa: E731
    same = lambda got, given: len(got) >= len(given) and all(g is o for g, o in zip(got, given))  # noqa: E731
    # offsets in every accepted form (converted ones pass again), given outputs of every row-output call
    ls, ts = e.f32(3, N), e.f32(3, N)
    assert same(pl.stack_batch(e.X, F, ls, ts), (ls, ts))
    for first in (np.array(F, np.int32), np.array(F, np.uint64), tuple(F)):
        assert torch.equal(pl.stack_batch(e.X, first)[1], ts)
    assert not ts[1].any().item() and ts[0].any().item()  # (the empty ensemble: a zero row)
    one = (e.f32(N), e.f32(2 * N))  # (_out: at least N samples)
    assert same(pl.stack_single(e.X, *one), one)
    given = rows_out(3)
    assert same(pl.jackknife_single(e.X, e.sel, *given), given) and given[2].tolist() == [5, 6, 6]
    given = rows_out(3)[:2]
    assert same(pl.subsample_sel(e.X, e.masks.astype(bool), 0.4, *given), given)
    assert tuple(pl.subsample_sel(e.X, e.masks, 0.4)[0].shape) == (3, N)
    for call, arg in ((pl.subsample_batch, e.masks), (pl.subsample_batch, e.masks.view(np.uint8)), (pl.bootstrap_batch, e.cnt),
                      (pl.weighted_stack_batch, e.w)):
        given = rows_out(3, 3)
        assert same(call(e.X, F, arg, *given), given) and (given[2][1] == 0).all() and (given[2] != 99).all()
    for call in (pl.jackknife_batch, pl2.jackknife_batch_two_stage):
        given = (e.f32(3, N), e.f32(3, N)) + rows_out(3, 3)
        assert same(call(e.X, F, e.sel, *given), given) and (given[4][1] == 0).all()
        got = call(e.X, F, e.sel, main=False)
        assert got[0] is None and got[1] is None and tuple(got[2].shape) == (3, 3, N) and (got[4] == given[4]).all()
    # coefficient sets: numpy in, numpy out; device tensor in, device tensor out
    x = pl.inverse(e.Y)
    assert isinstance(x, np.ndarray) and x.shape == (2, N) and not x.any()
    xd = pl.inverse(torch.from_numpy(e.Y).cuda())
    assert isinstance(xd, torch.Tensor) and xd.is_cuda and tuple(xd.shape) == (2, N)
    assert isinstance(pl.inverse_bands(e.Y, [(0, 2)]), np.ndarray)
    Xb, Qb = pl.inverse_bands(torch.from_numpy(e.Y).cuda(), [(0, 2), (1, 3)], quadrature=True)
    assert Xb.is_cuda and Qb.is_cuda and tuple(Xb.shape) == (2, 2, N)
    assert len(pl.stack_batch_bands(e.X, F, [(0, 2)], envelope=True)) == 4
    # rows as a view of a wider base, strided counts (they are copied), a given `out`
    wide = e.f32(3, 3, N + 8)
    wide[:, :, :N] = e.rows
    mtr = np.ones((3, 6), np.uint32)[:, ::2]
    out = e.f32(3, 2, N)
    assert pl.replica_bands(wide[:, :, :N], [0.25, 0.75], mtr, out=out) is out
    assert torch.equal(out, pl.replica_bands(e.rows, [0.25, 0.75]))
    fit = e.f64(3 * 3 * 4 + 5)  # (at least B M W 4 values)
    assert pl.stretch_rows(wide[:, :, :N], e.ref, 256.0, e.eps, e.win, mtr=mtr, out=fit) is fit
    cc, fit2 = pl.stretch_rows(e.rows, e.ref, 256.0, e.eps, e.win, cc=True)
    assert tuple(cc.shape) == (3, 3, 1, 5) and tuple(fit2.shape) == (3, 3, 1, 4) and not fit[36:].any().item()
    refs = e.f32(3, 2, N + 8)
    refs[:, :, :N] = e.rows[:, :2]
    sc = pl.trace_scores(e.X, F, refs[:, :, :N])
    assert tuple(sc.shape) == (2, 3, 7) and tuple(pl.trace_scores(e.X, F, e.rows[:, 0]).shape) == (1, 3, 7)  # ([B][N]: one reference row)
    assert len(pl.selective_stack_batch(e.X, F)) == 5
    # references: [N] and [1][N] for one ensemble, [B][N] for a batch
    r_ts, r_ls = e.rows[0, 0].contiguous(), e.rows[0, 1].contiguous()
    a, b = pl.convergence(e.X, r_ts, r_ls), pl.convergence(e.X, r_ts[None], r_ls[None])
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b)) and a[0].shape == (7,)
    own = pl.convergence_batch(e.X, F)
    given = pl.convergence_batch(e.X, np.array(F, np.uint64), ts, ls)  # (stack_batch's rows, handed in)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(own, given)) and own[0].shape == (7,)
    # x2 of exactly 2 N values
    x2 = torch.arange(2 * N, dtype=torch.float64, device="cuda")
    lo, to = e.f32(N), e.f32(N)
    pl.epilogue(x2, 4, lo, to)
    torch.cuda.synchronize()
    assert torch.equal(to, x2[:N].float()) and torch.equal(lo, (x2[N:] / 4).float())
    for name, names in STATS.items():
        st = getattr(pl2 if "two_stage" in name else pl, name)()
        assert tuple(st) == names and all(isinstance(v, int) for v in st.values()), name
