"""Helper of tests/test_dtw_rows_gpu.py and its child process: the rounds batch of the dynamic time warping call.  12 ensembles of 24 rows of
1501 samples under parameter set (iii) (Lmax = 127: 256 padded lag indices) over the four ranges of dtw_rows_ref.RANGES hold
(94 + 1 + 1 + 38) x 256 choice words a row, 137 KB, 3.3 MB an ensemble, so under TSPWS_PART_MB=16 (the smallest budget; the library reads it
once per process) tspws_hip_dtw_rows takes 3 rounds (5, 5 and 2 whole ensembles) where the default budget takes one.  As a program, argv[1] = an
.npz path: runs Plan.dtw_rows on that batch under the environment's budget and writes fit, lag and the stats there for the parent to
compare.  Prints DTW_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import dtw_rows_ref as dr

tspws = importlib.import_module("ts-pws_amd")

N = dr.N
RB, RM = 12, 24


def rounds_batch():
    rows, ref, mtr = dr.parity_batch(77, RB, RM)
    mtr[:] = 1
    mtr[5, ::4] = 0
    return rows, ref, mtr


def run(torch):
    """(fit, lag as numpy, stats) of the rounds batch."""
    rows, ref, mtr = rounds_batch()
    Lmax, b = dr.SETS["iii"]
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    out = pl.dtw_rows(torch.from_numpy(rows).cuda()[:, :, :N], torch.from_numpy(ref).cuda()[:, :N], dr.Z, dict(Lmax=Lmax, b=b), dr.RANGES, mtr=mtr)
    return out["fit"].cpu().numpy(), out["lag"].cpu().numpy(), pl.dtw_rows_stats()


if __name__ == "__main__":
    import torch

    fit, lag, st = run(torch)
    np.savez(sys.argv[1], fit=fit, lag=lag, rounds=st["rounds"])
    print("DTW_DONE", st["rounds"], flush=True)
