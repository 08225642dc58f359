"""Helper of tests/test_wxs_rows_gpu.py and its child process: the rounds batch of the wavelet cross-spectrum call.  48 ensembles of 9 rows
of 1501 samples hold (9 + 1) x 5968 complex coefficients each, 0.95 MB, so under TSPWS_PART_MB=16 (the smallest budget; the library reads it
once per process) tspws_hip_wxs_rows takes 3 rounds of whole ensembles where the default budget takes one.  As a program, argv[1] = an
.npz path: runs Plan.wxs_rows on that batch under the environment's budget and writes sums, fit and the stats there for the parent to
compare.  Prints WXS_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import wxs_rows_ref as wr

tspws = importlib.import_module("ts-pws_amd")

N = wr.N
RB, RM = 48, 9


def rounds_batch():
    rows, ref, mtr = wr.parity_batch(77, RB, RM)
    mtr[:] = 1
    mtr[5, ::4] = 0
    return rows, ref, mtr


def run(torch):
    """(sums, fit as numpy, stats) of the rounds batch on NaN-filled outputs, with the wrap rule."""
    rows, ref, mtr = rounds_batch()
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    bands = wr.parity_bands(wr.Frame.from_plan(pl))
    sums, fit = pl.wxs_rows(torch.from_numpy(rows).cuda()[:, :, :N], torch.from_numpy(ref).cuda()[:, :N], wr.Z, bands, wr.WINDOWS, mtr=mtr,
                            skip_wrapped=True, sums=True)
    return sums.cpu().numpy(), fit.cpu().numpy(), pl.wxs_rows_stats()


if __name__ == "__main__":
    import torch

    sums, fit, st = run(torch)
    np.savez(sys.argv[1], sums=sums, fit=fit, rounds=st["rounds"])
    print("WXS_DONE", st["rounds"], flush=True)
