"""Child process of tests/test_stack_batch_bands_gpu.py: the band-limited batched stack under TSPWS_PART_MB=16, which the library reads once per
process.  The batch of tests/batch_engine.batch at N = 8192 with Kmax = 4 unbiased: the ensembles of 5, 8 and 67 traces share the two-stage
pass, and the scale rows of their six sets (S x N doubles per set, twice that with the quadrature) exceed the budget, so the finish takes more
than one batch of sets (Plan.stack_batch_bands_stats).  Every row is held to tests/band_batch_ref.py at the parity figure.  Prints
BAND_BATCH_CHILD <worst ratios> <stats>; exits 1 on a row over 2e-6."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi
import band_batch_ref as bbr
import torch

TOL32 = 2e-6
N, SIZES = 8192, [1, 3, 5, 8, 0, 67]
assert os.environ.get("TSPWS_PART_MB") == "16"
tspws = importlib.import_module("ts-pws_amd")
assert tspws.load().tspws_hip_device_count() > 0
p = abi.default_params(unbiased=1, Kmax=4)
pl = tspws.Plan(tspws.resolve(p, N), N)
first = np.concatenate([[2], 2 + np.cumsum(SIZES)]).astype(np.int64)
X = abi.synth_traces(int(first[-1]), N, seed=21)
buf = torch.zeros((X.shape[0], N + 5), dtype=torch.float32, device="cuda")
buf[:, :N] = torch.from_numpy(X).cuda()
S, V = pl.S, pl.info.V
bands = [(0, S // 3 + 1), (S // 3 + 1, S - V - 2), (S - V - 2, S), (0, S), (1, 1)]
got = [t.cpu().numpy() for t in pl.stack_batch_bands(buf[:, :N], first, bands, envelope=True)]
st = pl.stack_batch_bands_stats()
assert st["two_stage_pass"] == 3 and st["looped"] == 2 and st["scales"] == S and st["quadrature"] == 1, st
assert S * N * 16 * 6 > 16 << 20 and st["finish_batches"] > 2 + st["rounds"], st   # the two single calls take one each; a round more than one
want = bbr.expected(abi.resolve(p, N), X, first, bands)
worst, bad = {}, []
for k, g, e in zip(("ls", "ts", "ls_env", "ts_env"), got, want):
    worst[k] = 0.0
    for idx in np.ndindex(e.shape[:-1]):
        if not e[idx].any():
            if g[idx].any():
                bad.append((k, idx, "not zero"))
        else:
            r = abi.relerr(g[idx], e[idx])
            worst[k] = max(worst[k], r)
            if not r <= TOL32:
                bad.append((k, idx, r))
print("BAND_BATCH_CHILD TSPWS_PART_MB=16 N = %d Kmax = 4 unbiased: bands %s | %s | %s%s" % (
    N, bands, ", ".join(f"{k} {v:.3g}" for k, v in worst.items()), st, f" | OVER {bad[:6]}" if bad else ""), flush=True)
sys.exit(1 if bad else 0)
