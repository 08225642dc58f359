#!/usr/bin/env python3
"""Bit-for-bit comparison of the batched entry points between two builds of the library: the parent's (ts-pws_amd/lib/variant_base.so, from
tools/build_base.sh) and the working tree's.  For each library and for TSPWS_PART_MB unset and = 16 a fresh child process (library by
TSPWS_LIB_PATH) runs the nine entry points -- stack_batch, jackknife_single, jackknife_batch, jackknife_batch_two_stage, convergence_batch,
subsample_batch_sel (masks given), subsample_batch (masks drawn after srand), bootstrap_batch (counts given, with the statistics) and
weighted_stack_batch -- on seeded inputs and stores every float output, count and Keff; the parent process compares the stored arrays byte
for byte and exits non-zero on any difference.

The masked replicas of ONE ensemble (resample.hip) get children of their own (`masked`): tspws_hip_jackknife, tspws_hip_stack_jackknife,
two-stage tspws_hip_subsample_sel and a two-shard jackknife_local + jackknife_finish on one device (the shards' rows added on the device, the
cut inside a run), with Kmax = 10, 33 and 70 traces, N = 4096 and 4001, and 9 / 15 / 17 / 40 columns (the direct walk's 12- and 16-column forms,
the snapshot form).  Engines: the default (the shipped libraries) and, with the sweeps builds (lib/variant_base_sweeps.so against
lib/libtspws_hip_sweeps.so), TSPWS_JK_DIRECT=0, TSPWS_JK_STAGES=5 and TSPWS_JK_PIPELINE=0 -- a fresh child each, at both budgets.
Children run one after the other, each under `timeout -k 10`; the first one that fails ends the run.

Shapes: 13 ensembles of 0-70 traces (one empty, one of 70 that straddles a 64-trace block, one of exactly 64), N = 4096 and N = 4001; the
single-stage parameter set and Kmax = 10, unbiased; 9 jackknife columns for the single-stage jackknives, 17 columns / masks (two column tiles
of the two-stage walk, three groups of 8 rows, the last holding one) for the others.  The count matrix: an all-zero row, a 0/1 row, one entry
of 255, otherwise 0..3; the weight matrix: an all-zero row, a row with a single weight, a 0/1 row, a row spanning 1e-6..1e6, otherwise
uniform in [0, 1).  A child fails unless the stats calls say that the shared paths ran (with the 16 MB budget: in more than one round).
usage: batch_ab.py [base.so new.so [base_sweeps.so new_sweeps.so]]      (children: batch_ab.py run out.npz, batch_ab.py masked out.npz)"""
import ctypes as C
import importlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES_MIXED = [1, 5, 33, 70, 0, 12, 64, 40, 17, 65, 28, 9, 30]   # single-stage under either parameter set: 1, 5, 9
SIZES_TWO = [10, 15, 33, 70, 0, 12, 64, 40, 17, 65, 28, 11, 30]  # every non-empty ensemble two-stage with Kmax = 10
NS = (4096, 4001)
C1, C2 = 9, 17


def bins_selection(sizes, C):
    """[C][T] delete-one selection: trace i of an ensemble sits in bin i % C, column c drops bin c (ensembles shorter than C: empty bins)."""
    sel = np.ones((C, sum(sizes)), np.int8)
    t = 0
    for m in sizes:
        for i in range(m):
            sel[i % C, t + i] = 0
        t += m
    return sel


def row_matrices(seed):
    """[C2][T] bootstrap counts and weights over the traces of SIZES_MIXED (docstring above)"""
    rng = np.random.default_rng(seed)
    T = sum(SIZES_MIXED)
    cnt = rng.integers(0, 4, (C2, T)).astype(np.uint8)
    cnt[0] = 0
    cnt[1] = rng.integers(0, 2, T)
    cnt[2, 7] = 255
    w = rng.random((C2, T))
    w[0] = 0
    w[1] = 0
    w[1, 40] = 0.75
    w[2] = rng.integers(0, 2, T)
    w[3] = 10.0 ** rng.uniform(-6, 6, T)
    return cnt, w


def child(path):
    import torch
    import abi
    tspws = importlib.import_module("ts-pws_amd")
    out = {}
    small = "TSPWS_PART_MB" in os.environ  # the budget that forces several rounds

    def keep(tag, *arrays):
        for k, a in enumerate(arrays):
            out[f"{tag}.{k}"] = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    for N in NS:
        pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)

        def params(two):
            pl.params.Kmax, pl.params.unbiased = (10, 1) if two else (0, 0)

        first_m = np.concatenate([[0], np.cumsum(SIZES_MIXED)]).astype(np.int64) + 2
        first_t = np.concatenate([[0], np.cumsum(SIZES_TWO)]).astype(np.int64) + 2
        X = tspws.synth(int(max(first_m[-1], first_t[-1])), N, seed=N)
        masks = (np.random.default_rng(N).random((C2, sum(SIZES_MIXED))) < 0.6).astype(np.int8)
        for two in (False, True):
            params(two)
            tag = f"N{N}.{'two' if two else 'one'}"
            n2 = sum(1 for m in SIZES_MIXED if two and m >= 10)
            n1 = sum(1 for m in SIZES_MIXED if m) - n2
            # stack_batch: mixed sizes
            keep(tag + ".stack", *pl.stack_batch(X, first_m))
            st = pl.batch_stats()
            # (the three single-stage ensembles of the two-stage set are too few traces for the many-trace pass: looped)
            assert st["two_stage_pass"] == n2 and st["empty"] == 1 and ((st["single_pass"], st["looped"]) == ((0, n1) if two else (n1, 0))), st
            # convergence_batch against the ensembles' own stacks, with the steps
            keep(tag + ".conv", *pl.convergence_batch(X, first_m, steps=True))
            st = pl.convergence_batch_stats()
            assert st["looped"] == 0 and st["single_steps"] > 0 and (st["two_stage_steps"] > 0) == two and st["rounds"] >= 1, st
            # subsample_batch with the masks given
            keep(tag + ".sub", *pl.subsample_batch(X, first_m, masks))
            st = pl.subsample_batch_stats()
            assert st["single_shared"] == n1 and st["two_stage_shared"] == n2 and st["looped"] == 0 and st["empty"] == 1, st
            # ... and with the masks drawn by the call itself, from a seeded rand()
            B = len(SIZES_MIXED)
            sl = torch.full((B, C2, N), float("nan"), dtype=torch.float32, device="cuda")
            st2 = torch.full((B, C2, N), float("nan"), dtype=torch.float32, device="cuda")
            sm = np.full((B, C2), 99, np.uint32)
            f = np.ascontiguousarray(first_m, dtype=np.uint64)
            pl.params.subsmpl_p = 0.6
            abi.srand(N + two)
            rc = pl.lib.tspws_hip_subsample_batch(pl.h, C.byref(pl.params), X.data_ptr(), X.stride(0), f.ctypes.data, B, C2, sl.data_ptr(), st2.data_ptr(),
                                                  sm.ctypes.data, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, pl.lib.tspws_hip_last_error()
            keep(tag + ".sub_drawn", sl, st2, sm)
            st = pl.subsample_batch_stats()
            assert st["single_shared"] == n1 and st["two_stage_shared"] == n2 and st["looped"] == 0, st
            if not two:
                assert st["rounds"] > 1 or not small, st  # (every ensemble single-stage: the rounds are those of the row batches)
                # bootstrap_batch (counts given, with the statistics) and weighted_stack_batch: the other two row batches
                cnt, w = row_matrices(N + 1)
                keep(tag + ".boot", *pl.bootstrap_batch(X, first_m, cnt, stats=True))
                st = pl.bootstrap_batch_stats()
                assert st["shared"] == n1 > 0 and st["empty"] == 1 and st["max_count"] == 255 and (st["rounds"] > 1 or not small), st
                keep(tag + ".weighted", *pl.weighted_stack_batch(X, first_m, w))
                st = pl.weighted_stack_batch_stats()
                assert st["shared"] == n1 > 0 and st["empty"] == 1 and (st["rounds"] > 1 or not small), st
                sel = bins_selection(SIZES_MIXED, C1)
                keep(tag + ".jkb", *pl.jackknife_batch(X, first_m, sel))
                st = pl.jackknife_batch_stats()
                assert st["shared"] == 12 and st["looped"] == 0 and st["empty"] == 1 and st["rounds"] >= 1, st
                keep(tag + ".jkb_nomain", *pl.jackknife_batch(X, first_m, sel, main=False)[2:])
                f0, f1 = int(first_m[3]), int(first_m[4])  # the ensemble of 70 traces alone
                keep(tag + ".jk1", *pl.jackknife_single(X[f0:f1], np.ascontiguousarray(sel[:, f0 - 2:f1 - 2])))
                keep(tag + ".jk1_many_classes", *pl.jackknife_single(X[f0:f1], np.ascontiguousarray(masks[:C1, f0 - 2:f1 - 2])))  # > 24 classes: no LDS
            else:
                sel = bins_selection(SIZES_TWO, C2)
                keep(tag + ".jkb2", *pl.jackknife_batch_two_stage(X, first_t, sel))
                st = pl.jackknife_batch_two_stage_stats()
                assert st["shared"] == 12 and st["looped"] == 0 and st["empty"] == 1 and st["tiles"] == 2 and st["rounds"] >= 1, st
                keep(tag + ".jkb2_nomain", *pl.jackknife_batch_two_stage(X, first_t, sel, main=False)[2:])
        pl.close()
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("AB_DONE", len(out), "arrays")


MASKED_MTR = (33, 70)
MASKED_C = (9, 15, 17, 40)
MASKED_ENGINES = (dict(TSPWS_JK_DIRECT="0"), dict(TSPWS_JK_STAGES="5"), dict(TSPWS_JK_PIPELINE="0"))  # of test_masked_replica_engines_agree


def child_masked(path):
    """the masked replicas of one ensemble: the four calls of resample.hip that build a MaskedPlan"""
    import torch
    import abi
    tspws = importlib.import_module("ts-pws_amd")
    out = {}

    def keep(tag, *arrays):
        for k, a in enumerate(arrays):
            out[f"{tag}.{k}"] = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    for N in NS:
        pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
        pl.params.Kmax, pl.params.unbiased = 10, 1
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for mtr in MASKED_MTR:
            X = tspws.synth(mtr, N, seed=N + mtr)
            rng = np.random.default_rng(N + mtr)
            for Cn in MASKED_C:
                tag = f"N{N}.m{mtr}.C{Cn}"
                sel = bins_selection([mtr], Cn)              # delete-one bins (Cn > mtr: the last columns keep every trace) ...
                sel[1] = rng.random(mtr) < 0.6               # ... and one column with runs of every length
                jl = torch.full((Cn, N), float("nan"), dtype=torch.float32, device="cuda")
                jt = torch.full((Cn, N), float("nan"), dtype=torch.float32, device="cuda")
                jm = np.full(Cn, 99, np.uint32)
                rc = pl.lib.tspws_hip_jackknife(pl.h, C.byref(pl.params), X.data_ptr(), X.stride(0), mtr, sel.ctypes.data, Cn, jl.data_ptr(), jt.data_ptr(),
                                                jm.ctypes.data, stream)
                assert rc == 0, pl.lib.tspws_hip_last_error()
                keep(tag + ".jk", jl, jt, jm)
                keep(tag + ".stack_jk", *pl.stack_jackknife(X, sel))
                K = int(np.ceil(mtr * 0.6))                  # subsample_sel: every mask with exactly ceil(mtr p) ones
                masks = np.zeros((Cn, mtr), np.int8)
                for c in range(Cn):
                    masks[c, rng.permutation(mtr)[:K]] = 1
                keep(tag + ".sub_sel", *pl.subsample_sel(X, masks, prob=0.6))
                # two shards on one device: the second shard starts inside a run; the shards' rows add up
                h = mtr // 2 + 1
                pl.jackknife_local(X[:h], 0, mtr, sel)
                rows0, main0 = pl.jackknife_buffer(Cn).clone(), pl.reduce_buffer(mtr).clone()
                pl.jackknife_local(X[h:], h, mtr, sel)
                pl.jackknife_buffer(Cn).add_(rows0)
                pl.reduce_buffer(mtr).add_(main0)
                ls = torch.empty(N, dtype=torch.float32, device="cuda")
                ts = torch.empty(N, dtype=torch.float32, device="cuda")
                lo = torch.zeros((Cn, N), dtype=torch.float32, device="cuda")
                to = torch.zeros((Cn, N), dtype=torch.float32, device="cuda")
                mo = np.zeros(Cn, np.uint32)
                pl.stack_finish(mtr, ls, ts)
                pl.jackknife_finish(mtr, sel, 0, Cn, lo, to, mo)
                keep(tag + ".sharded", ls, ts, lo, to, mo)
        pl.close()
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("AB_DONE", len(out), "arrays")


def compare(a, b):
    """(bytes compared, differing bytes) of two stored runs"""
    assert sorted(a.files) == sorted(b.files)
    nbytes = diff = 0
    for key in sorted(a.files):
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, key
        d = int((np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)).sum())
        nbytes += x.nbytes
        diff += d
        if d:
            print(f"  DIFF {key}: {d} of {x.nbytes} bytes")
        if x.dtype.kind == "f" and x.size and not np.isfinite(x).all():
            print(f"  (not finite in both: {key})")
    return nbytes, diff


def main():
    libdir = os.path.join(ROOT, "ts-pws_amd", "lib")
    default = [os.path.join(libdir, f) for f in ("variant_base.so", "libtspws_hip.so", "variant_base_sweeps.so", "libtspws_hip_sweeps.so")]
    libs = sys.argv[1:3] if len(sys.argv) >= 3 else default[:2]
    sweeps = sys.argv[3:5] if len(sys.argv) >= 5 else default[2:]
    # (child mode, the two libraries, switches): the batched entry points, then the masked replicas per engine
    runs = [("run", libs, {}), ("masked", libs, {})] + [("masked", sweeps, e) for e in MASKED_ENGINES]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for mode, pair, switches in runs:
            for budget in (None, "16"):
                res = []
                for k, lib in enumerate(pair):
                    env = dict(os.environ, TSPWS_LIB_PATH=os.path.abspath(lib), **switches)
                    env.pop("TSPWS_PART_MB", None)
                    if budget:
                        env["TSPWS_PART_MB"] = budget
                    path = os.path.join(tmp, f"{k}.npz")
                    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), mode, path], env=env, capture_output=True, text=True)
                    if r.returncode or "AB_DONE" not in r.stdout:
                        print(r.stdout[-3000:], r.stderr[-3000:])
                        sys.exit(f"child failed (status {r.returncode}): {mode} {lib} TSPWS_PART_MB={budget} {switches}")
                    res.append(np.load(path))
                nbytes, diff = compare(*res)
                what = " ".join(f"{k}={v}" for k, v in switches.items()) or "default engine"
                print(f"{mode} ({what}) TSPWS_PART_MB={budget or 'unset'}: {len(res[0].files)} arrays, {nbytes} bytes compared, {diff} differing bytes", flush=True)
                bad += diff
    print("shapes: ensembles", SIZES_MIXED, "(mixed) /", SIZES_TWO, "(two-stage), first[0] = 2, N in", NS, f"C = {C1} / {C2}, M = {C2}")
    print("masked: Kmax = 10, mtr in", MASKED_MTR, "C in", MASKED_C)
    print("libraries:", *[os.path.basename(p) for p in libs + sweeps])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "run":
        child(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "masked":
        child_masked(sys.argv[2])
    else:
        main()
