"""Single-stage jackknife on the GPU (tspws_hip_jackknife_single, tspws_main, Plan.jackknife_single, the CLI) against the trace-order
restatement of tests/jk_single_ref.py: replica c = the single-stage resampling body on mask row c with K = M = K_c."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import abi
import jk_single_ref as ref

pytestmark = pytest.mark.gpu

TOL32 = 2e-6
tspws = importlib.import_module("ts-pws_amd")
EXE = os.path.join(abi.ROOT, "ts-pws_amd", "bin", "ts_pws")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    return lib


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def check_replicas(got_ls, got_ts, got_mtr, want):
    wl, wt, wm = want
    np.testing.assert_array_equal(got_mtr, wm)
    for c in range(len(wm)):
        if wm[c]:
            assert abi.relerr(got_ts[c], wt[c]) < TOL32, c
            assert abi.relerr(got_ls[c], wl[c]) < TOL32, c
        else:
            assert not got_ts[c].any() and not got_ls[c].any(), c


# (params, mtr, N, (n, d), beg): few-trace and many-trace engines, N = 1501 and 16 501 (any-N spectral path), types -1 / -2 / -3,
# unbiased, wu = 1.3, fold + rm, Nmax < mtr, Kmax > mtr (single stage as well)
CASES = [
    (dict(), 24, 4096, (4, 1), 0.0),
    (dict(type=-2, unbiased=1), 300, 8192, (5, 2), 0.0),
    (dict(type=-3, wu=1.3), 40, 1501, (6, 5), 0.0),
    (dict(unbiased=1, fold=1, lrm=1, Nmax=50), 64, 16501, (4, 1), -0.5 * 16500),
    (dict(wu=1.3, lrm=1, Kmax=500), 30, 2048, (5, 2), 0.0),
]


@pytest.mark.parametrize("kw,mtr,N,nd,beg", CASES)
def test_tspws_main_replicas_match_the_restatement(lib, kw, mtr, N, nd, beg):
    n, d = nd
    X = abi.synth_traces(mtr, N, seed=mtr + N)
    times = ref.leap_times(mtr, seed=n + d)
    pj = abi.default_params(jackknife_n=n, jackknife_d=d, **kw)
    got = abi.run_main(lib.tspws_main, pj, X, beg=beg, times=times)
    assert got["rc"] == 0
    p, Xp, _ = ref.prologue(abi.default_params(**kw), X, beg=beg)
    sel = ref.selection(times[:Xp.shape[0]], n, d)
    check_replicas(got["jk_ls"], got["jk_ts"], got["jk_mtr"], ref.Restatement(p, Xp).replicas(sel))
    # the main outputs are those of the same call without jackknife, bit for bit
    plain = abi.run_main(lib.tspws_main, abi.default_params(**kw), X, beg=beg)
    np.testing.assert_array_equal(got["ls"], plain["ls"])
    np.testing.assert_array_equal(got["tsPWS"], plain["tsPWS"])
    np.testing.assert_array_equal(got["sigall"], plain["sigall"])


def test_empty_replica_and_missing_start_times(lib, torch):
    mtr, N = 30, 2048
    X = abi.synth_traces(mtr, N, seed=3)
    jan = (1262304000 + 3600 * np.arange(mtr)).astype(np.int64)  # every trace in bin 0 of n = 4
    pj = abi.default_params(jackknife_n=4, jackknife_d=1)
    got = abi.run_main(lib.tspws_main, pj, X, times=jan)
    assert got["rc"] == 0
    np.testing.assert_array_equal(got["jk_mtr"], [0, mtr, mtr, mtr])
    p, Xp, _ = ref.prologue(abi.default_params(), X)
    check_replicas(got["jk_ls"], got["jk_ts"], got["jk_mtr"], ref.Restatement(p, Xp).replicas(ref.selection(jan, 4, 1)))
    # K_c = 0 through the device call: rows that held something come back zero
    pl = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    Xd = torch.from_numpy(X).cuda()
    ls_out = torch.full((4, N), 7.0, dtype=torch.float32, device="cuda")
    ts_out = torch.full((4, N), 7.0, dtype=torch.float32, device="cuda")
    mtr_out = np.full(4, 99, np.uint32)
    pl.jackknife_single(Xd, ref.selection(jan, 4, 1), ls_out, ts_out, mtr_out)
    torch.cuda.synchronize()
    assert not (ls_out[0] != 0).any().item() and not (ts_out[0] != 0).any().item() and mtr_out[0] == 0
    np.testing.assert_array_equal(ts_out[1:].cpu().numpy(), got["jk_ts"][1:])
    # no start times (zeros, or none at all): replicas untouched, main outputs produced
    for t in (np.zeros(mtr, np.int64), None):
        z = abi.run_main(lib.tspws_main, pj, X, times=t)
        assert z["rc"] == 0 and not z["jk_ts"].any() and not z["jk_ls"].any() and not z["jk_mtr"].any() and z["tsPWS"].any()


def test_matches_the_subsampling_engine(lib, torch):
    """tsPWS_out[c] == tspws_hip_subsample_sel on mask row c alone (M = 1) with ceil(mtr * subsmpl_p) == K_c."""
    mtr, N = 120, 4096
    X = abi.synth_traces(mtr, N, seed=12)
    times = ref.leap_times(mtr, seed=4)
    sel = ref.selection(times, 5, 2)
    p = tspws.resolve(abi.default_params(unbiased=1), N)
    pl = tspws.Plan(p, N)
    Xd = torch.from_numpy(X).cuda()
    ls_out, ts_out, mtr_out = pl.jackknife_single(Xd, sel)
    torch.cuda.synchronize()
    ts_out = ts_out.cpu().numpy()
    for c in range(sel.shape[0]):
        q = tspws.t_tsPWS.from_buffer_copy(p)
        q.subsmpl_N, q.subsmpl_p = 1, (int(mtr_out[c]) - 0.5) / mtr
        lo = torch.zeros(N, dtype=torch.float32, device="cuda")
        to = torch.zeros(N, dtype=torch.float32, device="cuda")
        row = np.ascontiguousarray(sel[c:c + 1])
        tspws.check(lib.tspws_hip_subsample_sel(pl.h, C.byref(q), Xd.data_ptr(), N, mtr, 1, row.ctypes.data, lo.data_ptr(), to.data_ptr(), None),
                    "subsample_sel")
        torch.cuda.synchronize()
        assert abi.relerr(ts_out[c], to.cpu().numpy()) < TOL32, c


def test_cabi_many_classes_and_two_stage_refusal(lib, torch):
    mtr, N, Cn = 60, 2048, 7
    X = abi.synth_traces(mtr, N, seed=21)
    rng = np.random.default_rng(8)
    sel = (rng.random((Cn, mtr)) < 0.55).astype(np.int8)  # ~60 classes: more than the LDS form of the finish kernel holds
    sel[3, :] = 0
    assert tspws.selection_classes(sel)[1].shape[1] > 24
    p = tspws.resolve(abi.default_params(type=-3, unbiased=1), N)
    pl = tspws.Plan(p, N)
    Xd = torch.from_numpy(X).cuda()
    jl = torch.zeros((Cn, N), dtype=torch.float32, device="cuda")
    jt = torch.zeros((Cn, N), dtype=torch.float32, device="cuda")
    jm = np.zeros(Cn, np.uint32)
    tspws.check(lib.tspws_hip_jackknife_single(pl.h, C.byref(pl.params), Xd.data_ptr(), N, mtr, sel.ctypes.data, Cn, jl.data_ptr(), jt.data_ptr(),
                                               jm.ctypes.data, None), "jackknife_single")
    check_replicas(jl.cpu().numpy(), jt.cpu().numpy(), jm, ref.Restatement(p, X).replicas(sel))
    # a two-stage parameter set is refused (tspws_hip_jackknife takes it)
    q = tspws.t_tsPWS.from_buffer_copy(pl.params)
    q.Kmax = 4
    assert lib.tspws_hip_jackknife_single(pl.h, C.byref(q), Xd.data_ptr(), N, mtr, sel.ctypes.data, Cn, jl.data_ptr(), jt.data_ptr(),
                                          jm.ctypes.data, None) == -1


CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import abi, jk_single_ref as ref
tspws = importlib.import_module("ts-pws_amd")
a = json.loads(sys.argv[1])
X = abi.synth_traces(a["mtr"], a["N"], seed=a["seed"])
times = ref.leap_times(a["mtr"], seed=a["tseed"])
r = abi.run_main(tspws.load().tspws_main, abi.default_params(**a["kw"]), X, times=times)
assert r["rc"] == 0
np.savez(a["out"], jk_ls=r["jk_ls"], jk_ts=r["jk_ts"], jk_mtr=r["jk_mtr"], ls=r["ls"], tsPWS=r["tsPWS"])
"""


def run_child(tmp_path, env, **a):
    a["out"] = str(tmp_path / "child.npz")
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=abi.ROOT, here=HERE), json.dumps(a)], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(a["out"])


def test_batches_are_bit_identical(lib, tmp_path):
    """n = 16, d = 3 (C = 560): with TSPWS_PART_MB=16 the traces are transformed in several batches and the replicas finished in
    several batches; the rows are those of the unbatched call bit for bit."""
    a = dict(mtr=300, N=1501, seed=5, tseed=9, kw=dict(jackknife_n=16, jackknife_d=3, unbiased=1))
    X = abi.synth_traces(a["mtr"], a["N"], seed=a["seed"])
    times = ref.leap_times(a["mtr"], seed=a["tseed"])
    full = abi.run_main(lib.tspws_main, abi.default_params(**a["kw"]), X, times=times)
    assert full["rc"] == 0 and len(full["jk_mtr"]) == 560
    small = run_child(tmp_path, dict(TSPWS_PART_MB="16"), **a)
    for k in ("jk_ls", "jk_ts", "jk_mtr"):
        np.testing.assert_array_equal(small[k], full[k])
    sel = ref.selection(times, 16, 3)
    R = ref.Restatement(abi.resolve(abi.default_params(**a["kw"]), a["N"]), X)
    for c in (0, 1, 137, 559):
        ls, ts, K = R.replica(sel[c])
        assert full["jk_mtr"][c] == K and abi.relerr(full["jk_ts"][c], ts) < TOL32 and abi.relerr(full["jk_ls"][c], ls) < TOL32


def test_plan_jackknife_single(lib, torch):
    mtr, N = 50, 3000
    X = abi.synth_traces(mtr, N, seed=30)
    times = ref.leap_times(mtr, seed=2)
    got = abi.run_main(lib.tspws_main, abi.default_params(wu=1.3, jackknife_n=5, jackknife_d=2), X, times=times)
    pl = tspws.Plan(tspws.resolve(abi.default_params(wu=1.3), N), N)
    Xd = torch.from_numpy(X).cuda()
    sel = tspws.jackknife_selection(times, 5, 2)
    jl, jt, jm = pl.jackknife_single(Xd, sel)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(jm, got["jk_mtr"])
    np.testing.assert_array_equal(jl.cpu().numpy(), got["jk_ls"])
    np.testing.assert_array_equal(jt.cpu().numpy(), got["jk_ts"])
    Cn = sel.shape[0]
    bad = [
        lambda: pl.jackknife_single(Xd.double(), sel),                                    # traces not float32
        lambda: pl.jackknife_single(Xd, sel[:, :-1]),                                     # selection of another ensemble
        lambda: pl.jackknife_single(Xd, sel.astype(np.float64)),                          # selection not int8
        lambda: pl.jackknife_single(Xd, sel[0]),                                          # selection not 2-D
        lambda: pl.jackknife_single(Xd, sel, ls_out=torch.empty((Cn, N + 1), device="cuda")),
        lambda: pl.jackknife_single(Xd, sel, ts_out=torch.empty((Cn, N), dtype=torch.float64, device="cuda")),
        lambda: pl.jackknife_single(Xd, sel, mtr_out=np.zeros(Cn, np.int32)),
        lambda: pl.jackknife_single(Xd, sel, mtr_out=np.zeros(Cn + 1, np.uint32)),
    ]
    for f in bad:
        with pytest.raises(tspws.TspwsError):
            f()


def test_cli_single_stage_jackknife(lib, tmp_path, golden):
    g = golden["example32"]
    X = g["traces"]
    mtr, n = X.shape
    names = []
    for i, x in enumerate(X):
        path = tmp_path / f"t{i:03d}.sac"
        abi.write_sac(str(path), x, float(g["dt"]), float(g["beg"]), year=2010, jday=1 + 11 * i, kstnm="CAN")
        names.append(str(path))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    times = (1262304000 + 86400 * 11 * np.arange(mtr)).astype(np.int64)
    want = abi.run_main(lib.tspws_main, abi.default_params(jackknife_n=4, jackknife_d=1), X, dt=float(g["dt"]), beg=float(g["beg"]), times=times)
    assert want["rc"] == 0 and want["jk_mtr"].all()
    for args in (("osac=j1",), ("osac=j1b", "obin")):
        r = subprocess.run([EXE, "list.txt", *args, "jackknife_n=4", "jackknife_d=1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    for c in range(4):
        ts, ls = abi.read_sac(tmp_path / f"ts_pws_j1_subsmpl_{c}.sac"), abi.read_sac(tmp_path / f"tl_j1_subsmpl_{c}.sac")
        np.testing.assert_array_equal(ts["data"], want["jk_ts"][c])
        np.testing.assert_array_equal(ls["data"], want["jk_ls"][c])
        assert ts["f"][40] == float(want["jk_mtr"][c])
    for pre, key in (("ts_pws", "jk_ts"), ("tl", "jk_ls")):
        raw = open(tmp_path / f"{pre}_j1b_subsmpl.bin", "rb").read()
        np.testing.assert_array_equal(np.frombuffer(raw, "<i8", 4, 116), want["jk_mtr"])
        np.testing.assert_array_equal(np.frombuffer(raw, "<f4", 4 * n, 116 + 8 * 4).reshape(4, n), want[key])
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=60).stdout
    assert "TwoStage only" not in usage


def test_device_list_runs_it_on_the_first_device(lib, tmp_path):
    a = dict(mtr=90, N=2048, seed=71, tseed=3, kw=dict(jackknife_n=5, jackknife_d=2))
    X = abi.synth_traces(a["mtr"], a["N"], seed=a["seed"])
    one = abi.run_main(lib.tspws_main, abi.default_params(**a["kw"]), X, times=ref.leap_times(a["mtr"], seed=a["tseed"]))
    two = run_child(tmp_path, dict(TSPWS_DEVICES="0,0", TSPWS_COMM="local"), **a)
    for k in ("jk_ls", "jk_ts", "jk_mtr", "ls", "tsPWS"):
        np.testing.assert_array_equal(two[k], one[k])
    assert one["jk_mtr"].all()
