"""Helper of tests/test_mwcs_rows_gpu.py and its child process: the rounds batch of the moving-window cross-spectrum call.  12 ensembles of
9 rows of 1501 samples under parameter set (iii) (L = 16, hop = 1: J = 2565 windows, Qx = 5 bins in 16 padded columns) hold
(9 + 1) x 2565 x 16 doubles of spectra and 9 x 2565 x 3 of window results each, 3.8 MB, so under TSPWS_PART_MB=16 (the smallest budget; the
library reads it once per process) tspws_hip_mwcs_rows takes 3 rounds of whole ensembles where the default budget takes one.  As a
program, argv[1] = an .npz path: runs Plan.mwcs_rows on that batch under the environment's budget and writes fit, win and the stats there
for the parent to compare.  Prints MWCS_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import mwcs_rows_ref as mr

tspws = importlib.import_module("ts-pws_amd")

N = mr.N
RB, RM = 12, 9


def rounds_batch():
    rows, ref, mtr = mr.parity_batch(77, RB, RM)
    mtr[:] = 1
    mtr[5, ::4] = 0
    return rows, ref, mtr


def run(torch):
    """(fit, win as numpy, stats) of the rounds batch."""
    rows, ref, mtr = rounds_batch()
    par, ranges = mr.SETS["iii"]
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    out = pl.mwcs_rows(torch.from_numpy(rows).cuda()[:, :, :N], torch.from_numpy(ref).cuda()[:, :N], mr.Z, par.kwargs(), ranges, mtr=mtr, win=True)
    return out["fit"].cpu().numpy(), out["win"].cpu().numpy(), pl.mwcs_rows_stats()


if __name__ == "__main__":
    import torch

    fit, win, st = run(torch)
    np.savez(sys.argv[1], fit=fit, win=win, rounds=st["rounds"])
    print("MWCS_DONE", st["rounds"], flush=True)
