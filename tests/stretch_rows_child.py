"""Helper of tests/test_stretch_rows_gpu.py and its child process: the batches of the GPU tests.  The rounds batch -- 48 ensembles of 33
rows of 1501 samples, E = 49 (a partial last tile of 16 stretches), the three windows -- needs about 0.47 MB per ensemble at 16 stretches, so
under TSPWS_PART_MB=16 (the smallest budget; the library reads it once per process) the call takes 2 rounds of whole ensembles (35 + 13)
and walks the padded grid of 64 in 4 and in 2 chunks.  As a program, argv[1] = an .npz path: runs Plan.stretch_rows on that batch under the
environment's budget and writes cc, fit and the stats there for the parent to compare.  Prints STRETCH_DONE <rounds> <chunks>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import stretch_rows_ref as srr

tspws = importlib.import_module("ts-pws_amd")

N = srr.N
RB, RM, RE = 48, 33, 49


def parity_batch(seed, B=3, M=33):
    """(rows float32 [B][M][N + 3], ref float32 [B][N + 1], counts uint32 [B][M]) with NaN pad columns: ensemble b has its own wavelet; row m
    is the analytically stretched wavelet (eps0 cycling through seven values) plus seeded noise of sigma 0, 0.2 or 1 (m % 3), scaled by
    1e-6 .. 1e2; row (0, 5) is all zero; the reference of ensemble 1 is zero inside [3, 611); the counts leave out 0 / 16 / 32 rows."""
    rng = np.random.default_rng(seed)
    rows = np.full((B, M, N + 3), np.nan, np.float32)
    ref = np.full((B, N + 1), np.nan, np.float32)
    t = np.arange(N, dtype=np.float64) - srr.Z
    eps0 = (0.0037, -0.00612, 0.0, 0.0081, -0.0029, 0.0011, -0.0093)
    for b in range(B):
        a = srr.wavelet(1000 * seed + b)
        ref[b, :N] = a(t)
        for m in range(M):
            x = a(t * (1 + eps0[m % len(eps0)])) + (0.0, 0.2, 1.0)[m % 3] * rng.standard_normal(N)
            rows[b, m, :N] = x * 10.0 ** rng.uniform(-6, 2)
    rows[0, 5, :N] = 0
    if B > 1:
        ref[1, 3:611] = 0
    mtr = np.full((B, M), 7, np.uint32)
    if B > 2:
        mtr[1, 1:32:2] = 0   # 16 rows left out: 17 take part
        mtr[2] = 0
        mtr[2, 20] = 3       # one row takes part
    return rows, ref, mtr


def rounds_batch():
    rows, ref, mtr = parity_batch(77, RB, RM)
    mtr[:] = 1
    mtr[5, ::4] = 0
    return rows, ref, mtr


def run(torch):
    """(cc, fit as numpy, stats) of the rounds batch on NaN-filled outputs."""
    rows, ref, mtr = rounds_batch()
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    eps = tspws.stretch_grid(0.012, RE)
    cc, fit = pl.stretch_rows(torch.from_numpy(rows).cuda()[:, :, :N], torch.from_numpy(ref).cuda()[:, :N], srr.Z, eps, srr.WINDOWS, mtr=mtr, cc=True)
    return cc.cpu().numpy(), fit.cpu().numpy(), pl.stretch_rows_stats()


if __name__ == "__main__":
    import torch

    cc, fit, st = run(torch)
    np.savez(sys.argv[1], cc=cc, fit=fit, rounds=st["rounds"], chunks=st["chunks"])
    print("STRETCH_DONE", st["rounds"], st["chunks"], flush=True)
