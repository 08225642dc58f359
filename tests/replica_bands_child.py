"""Helper of tests/test_replica_bands_gpu.py and its child process: the batch of the rounds test -- 320 ensembles of 9 replicas of 1501
samples, 17.3 MB of rows, so that under TSPWS_PART_MB=16 (the smallest budget; the library reads it once per process) the call takes 2
rounds of whole ensembles.  As a program, argv[1] = an .npz path: runs Plan.replica_bands on the batch under the environment's budget and
writes the bands and the round count there for the parent to compare.  Prints BANDS_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi

tspws = importlib.import_module("ts-pws_amd")

B, M, N = 320, 9, 1501
QS = [0, 0.025, 0.16, 1 / 3, 0.5, 0.84, 0.975, 1]


def batch():
    """(rows float32 [B][M][N], counts uint32 [B][M]): seeded normals; a few counts 0, ensemble 7 without a participating replica."""
    rng = np.random.default_rng(2024)
    rows = rng.standard_normal((B, M, N)).astype(np.float32)
    mtr = (rng.random((B, M)) < 0.8).astype(np.uint32) * 5
    mtr[7] = 0
    return rows, mtr


def run(torch):
    """(bands as numpy, stats) of the batch on a NaN-filled output."""
    rows, mtr = batch()
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    out = torch.full((B, len(QS), N), float("nan"), dtype=torch.float32, device="cuda")
    got = pl.replica_bands(torch.from_numpy(rows).cuda(), QS, mtr, out=out)
    assert got is out
    return out.cpu().numpy(), pl.replica_bands_stats()


if __name__ == "__main__":
    import torch

    bands, st = run(torch)
    assert st["lds"] == B - 1 and st["empty"] == 1 and st["global"] == 0, st
    np.savez(sys.argv[1], bands=bands, rounds=st["rounds"])
    print("BANDS_DONE", st["rounds"], flush=True)
