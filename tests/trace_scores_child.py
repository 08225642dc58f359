"""Helper of tests/test_trace_scores_gpu.py and its child process: the batch of the rounds test -- 2 ensembles of 64 000 synthetic traces
of 1501 samples, one column segment each: 128 000 slots of 128 bytes of partial sums + 32 000 group entries of 16 bytes = 16.9 MB, so that
under TSPWS_PART_MB=16 (the smallest budget; the library reads it once per process) the call takes 2 rounds of whole ensembles.  As a
program, argv[1] = an .npz path: runs Plan.trace_scores on the batch under the environment's budget and writes the scores, the energies
and the stats there for the parent to compare.  Prints SCORES_DONE <rounds>."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi

tspws = importlib.import_module("ts-pws_amd")

N, M = 1501, 64000
FIRST = np.array([0, M, 2 * M])


def run(torch):
    """(scores [2][3][2 M], energy [2 M]) as numpy and the stats: every trace against two rows of its own ensemble."""
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    x = tspws.synth(2 * M, N, seed=77)
    refs = torch.stack([x[0:2], x[M:M + 2]]).contiguous()
    scores, energy = pl.trace_scores(x, FIRST, refs, energy=True)
    return scores.cpu().numpy(), energy.cpu().numpy(), pl.trace_scores_stats()


if __name__ == "__main__":
    import torch

    scores, energy, st = run(torch)
    np.savez(sys.argv[1], scores=scores, energy=energy, rounds=st["rounds"], vec=st["vec"], segments=st["segments"])
    print("SCORES_DONE", st["rounds"], flush=True)
