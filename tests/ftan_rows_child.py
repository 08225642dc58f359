"""Helper of tests/test_ftan_rows_gpu.py and its child process: the rounds batch of the group-arrival call.  48 ensembles of 9 rows of 1501
samples hold 9 x 5968 complex coefficients each, 0.86 MB, so under TSPWS_PART_MB=16 (the smallest budget; the library reads it once per
process) tspws_hip_ftan_rows takes 3 rounds of whole ensembles where the default budget takes one.  The ensembles alternate between two
window sets (two classes) and have a noise range.  As a program, argv[1] = an .npz path: runs Plan.ftan_rows on that batch under the
environment's budget and writes peaks, noise and the stats there for the parent to compare.  Prints FTAN_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import ftan_rows_ref as fr_

tspws = importlib.import_module("ts-pws_amd")

N = fr_.N
RB, RM, RP = 48, 9, 3


def rounds_batch():
    rows, mtr = fr_.parity_batch(77, RB, RM)
    mtr[:] = 1
    mtr[5, ::4] = 0
    win = fr_.PWIN[np.arange(RB) % 2]
    noise = fr_.PNOISE[np.arange(RB) % 2]
    return rows, mtr, win, noise


def run(torch):
    """(peaks, noise as numpy, stats) of the rounds batch on NaN-filled outputs, with the wrap rule."""
    rows, mtr, win, noise = rounds_batch()
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    peaks, nz = pl.ftan_rows(torch.from_numpy(rows).cuda()[:, :, :N], fr_.Z, win, P=RP, noise=noise, mtr=mtr, skip_wrapped=True)
    return peaks.cpu().numpy(), nz.cpu().numpy(), pl.ftan_rows_stats()


if __name__ == "__main__":
    import torch

    peaks, nz, st = run(torch)
    np.savez(sys.argv[1], peaks=peaks, noise=nz, rounds=st["rounds"])
    print("FTAN_DONE", st["rounds"], flush=True)
