"""Helper of the batched convergence-curve tests (tspws_hip_convergence_batch, Plan.convergence_batch): the batch on the device and the
expected curves of every ensemble from the oracle's tspws_main on that ensemble alone.

The oracle gets an explicit reference trace R_b per ensemble (in->reference): it then uses R_b for both curves, so the expected values do
not depend on float-rounded final stacks; the device reference arrays hold row b = R_b for both ref_ts and ref_ls.  Expected curves are
computed once per (parameters, shape) and shared, unchanged, by the tests that need them.

As a script (child process of the small-budget test, which sets TSPWS_PART_MB before the library reads it):
    python conv_batch_ref.py '<json: kw, sizes, N, first0, pad>' out.npz
"""
import importlib
import json
import sys

import numpy as np

import abi

TOL32 = 2e-6   # float step arrays, relative per row (tests/test_hip_parity.py)
PAD_FILL = 1e30  # what the ld - N padding columns of the trace buffer hold: read into any sum, it shows

_expected = {}


def offsets(sizes, first0):
    return np.concatenate([[first0], first0 + np.cumsum(sizes)]).astype(np.int64)


def host_traces(sizes, N, first0, seed):
    """All rows of the trace array (the first0 rows in front belong to no ensemble): noise + packet, so no step's stack is zero."""
    return abi.synth_traces(first0 + int(sum(sizes)), N, seed=seed)


def references(B, N, seed):
    """R_b: one more noise + packet trace per ensemble, [B][N] float32."""
    return np.stack([abi.synth_traces(1, N, seed=seed + 977 + b)[0] for b in range(B)])


def expected(kw, sizes, N, first0, seed):
    """Per ensemble (None: empty) the oracle's curves and step arrays with R_b as the reference; every value finite."""
    key = (json.dumps(kw, sort_keys=True), tuple(sizes), N, first0, seed)
    if key not in _expected:
        X, R, f = host_traces(sizes, N, first0, seed), references(len(sizes), N, seed), offsets(sizes, first0)
        out = []
        for b, m in enumerate(sizes):
            if not m:
                out.append(None)
                continue
            r = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(convergence=1, AllSteps=1, **kw), X[f[b]:f[b + 1]], reference=R[b])
            assert r["rc"] == 0
            e = {k: r[k] for k in ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps")}
            for k, v in e.items():
                assert v.shape[0] == m and np.isfinite(v).all(), (b, k)
                v.setflags(write=False)
            out.append(e)
        _expected[key] = out
    return _expected[key]


def device_traces(torch, X, pad):
    """[rows][N] view of a [rows][N + pad] cuda buffer whose padding columns hold PAD_FILL."""
    rows, N = X.shape
    buf = torch.full((rows, N + pad), PAD_FILL, dtype=torch.float32, device="cuda")
    buf[:, :N] = torch.from_numpy(X).cuda()
    return buf, buf[:, :N]


def run(torch, kw, sizes, N, first0, pad, seed, refs=True):
    """The batched call with steps on the seeded traces.  refs=True: rows R_b; refs=None: the call's default references."""
    tspws = importlib.import_module("ts-pws_amd")
    p = tspws.resolve(abi.default_params(**kw), N)
    pl = tspws.Plan(p, N)
    X = host_traces(sizes, N, first0, seed)
    buf, tr = device_traces(torch, X, pad)
    f = offsets(sizes, first0)
    R = torch.from_numpy(references(len(sizes), N, seed)).cuda() if refs else None
    ts_sim, ts_mis, ls_sim, ls_mis, ts_steps, ls_steps = pl.convergence_batch(tr, f, R, R, steps=True)
    torch.cuda.synchronize()
    assert bool((buf[:, N:] == PAD_FILL).all()) and np.array_equal(tr.cpu().numpy(), X)  # the input is read only
    return dict(plan=pl, p=p, traces=tr, buf=buf, first=f, R=R, stats=pl.convergence_batch_stats(), conv_tsPWS_sim=ts_sim, conv_tsPWS_misfit=ts_mis,
                conv_ls_sim=ls_sim, conv_ls_misfit=ls_mis, conv_ts_steps=ts_steps.cpu().numpy(), conv_ls_steps=ls_steps.cpu().numpy())


def compare(got, want, tag=""):
    """The bounds of test_convergence_vs_oracle for one ensemble: similarities 1e-9 absolute, misfits 1e-7 max|expected| + 1e-18, both step
    arrays TOL32 relative per row.  Prints every figure before it asserts."""
    for k in ("conv_ls_sim", "conv_tsPWS_sim"):
        err = float(np.max(np.abs(got[k] - want[k])))
        print(tag, k, "abs err", err)
        assert np.isfinite(got[k]).all() and err < 1e-9, (tag, k, err)
    for k in ("conv_ls_misfit", "conv_tsPWS_misfit"):
        err, bound = float(np.max(np.abs(got[k] - want[k]))), 1e-7 * float(np.max(np.abs(want[k]))) + 1e-18
        print(tag, k, "abs err", err, "bound", bound)
        assert np.isfinite(got[k]).all() and err <= bound, (tag, k, err, bound)
    for k in ("conv_ts_steps", "conv_ls_steps"):
        assert np.isfinite(got[k]).all(), (tag, k)
        err = max(abi.relerr(a, b) for a, b in zip(got[k], want[k]))
        print(tag, k, "worst row relerr", err)
        assert err < TOL32, (tag, k, err)


def ensemble(r, first, b):
    """Entries of ensemble b of a batch result (the keys of `compare`)."""
    lo, hi = int(first[b] - first[0]), int(first[b + 1] - first[0])
    return {k: r[k][lo:hi] for k in ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps")}


def check_written(r, sizes):
    """The binding fills curves and step arrays with NaN before the call: every entry has been written."""
    T = int(sum(sizes))
    for k in ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps"):
        assert r[k].shape[0] == T and not np.isnan(r[k]).any(), k


if __name__ == "__main__":
    sys.path.insert(0, abi.ROOT)
    import torch
    a = json.loads(sys.argv[1])
    r = run(torch, a["kw"], a["sizes"], a["N"], a["first0"], a["pad"], a["seed"])
    np.savez(sys.argv[2], stats=np.array([r["stats"][k] for k in ("single_steps", "two_stage_steps", "rows", "rounds", "looped", "empty")]),
             **{k: r[k] for k in ("conv_tsPWS_sim", "conv_tsPWS_misfit", "conv_ls_sim", "conv_ls_misfit", "conv_ts_steps", "conv_ls_steps")})
    print("CONV_BATCH_DONE")
