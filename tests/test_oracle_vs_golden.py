"""Pin the oracle (oracle/tspws_oracle.c) against the golden vectors produced by
the reference itself (tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest

import abi

TOL = 1e-11  # oracle and reference are both FP64; only summation grouping / FMA contraction differ


def frame_names(g):
    return sorted({k.split("/")[0] for k in g["frames"].files})


def test_frame_tables(golden):
    g = golden["frames"]
    for name in frame_names(golden):
        f = abi.OracleFrame(int(g[f"{name}/type"]), int(g[f"{name}/J"]), int(g[f"{name}/V"]), int(g[f"{name}/N"]),
                            float(g[f"{name}/s0"]), float(g[f"{name}/b0"]), float(g[f"{name}/w0"]))
        assert f.S == int(g[f"{name}/S"]), name
        np.testing.assert_array_equal(f.L, g[f"{name}/L"], name)
        np.testing.assert_array_equal(f.c, g[f"{name}/c"], name)
        np.testing.assert_array_equal(f.cd, g[f"{name}/cd"], name)
        np.testing.assert_array_equal(f.D, g[f"{name}/D"], name)
        np.testing.assert_array_equal(f.scale, g[f"{name}/scale"], name)  # same repeated product -> bit equal
        assert f.Cpsi == float(g[f"{name}/Cpsi"]), name
        w, wd = f.taps()
        off = np.concatenate([[0], np.cumsum(f.L)]).astype(np.int64)
        e = g[f"{name}/w_head"].shape[1]
        for s in range(f.S):
            ws = w[off[s]:off[s + 1]]
            np.testing.assert_allclose(ws[:e], g[f"{name}/w_head"][s], rtol=1e-14, atol=1e-300, err_msg=name)
            np.testing.assert_allclose(ws[-e:], g[f"{name}/w_tail"][s], rtol=1e-14, atol=1e-300, err_msg=name)
            np.testing.assert_allclose(wd[off[s]:off[s] + e], g[f"{name}/wd_head"][s], rtol=1e-14, atol=1e-300, err_msg=name)
            assert abs(ws.sum() - g[f"{name}/w_sum"][s]) <= 1e-12 * max(1.0, np.abs(ws).sum()), name


def test_known_answers_from_survey():
    """SURVEY.md 8(c) [measured on the reference]."""
    f = abi.OracleFrame(N=131072, J=14)
    assert f.Cpsi == pytest.approx(0.29982027317664373, rel=1e-15)
    w, _ = f.taps()
    assert w[10] == pytest.approx(0.53112596601359841 + 0j, rel=1e-14)
    assert f.ncoef == 524256 and f.ntaps == 1383505
    assert abi.OracleFrame(N=2048, J=5, w0=2 * np.pi).Cpsi == pytest.approx(0.25329497516446658, rel=1e-15)
    assert abi.OracleFrame(type=-3, N=2048, J=5, V=2, s0=1.0, b0=0.5, w0=2 ** 0.5).Cpsi == pytest.approx(2.3632718012073544, rel=1e-15)


def test_parameter_resolution(golden):
    g = golden["mains"]
    names = sorted({k.split("/")[0] for k in g.files if "/in/" in k})
    assert len(names) >= 25
    for name in names:
        p = abi.t_tsPWS()
        for k in [k for k in g.files if k.startswith(f"{name}/in/")]:
            setattr(p, k.split("/")[-1], g[k].item())
        x = g["X"] if str(g[f"{name}/input"]) == "X" else g["Xodd"] if str(g[f"{name}/input"]) == "Xodd" else g[f"{name}/x"]
        q = abi.resolve(p, x.shape[1], float(g[f"{name}/dt"]))
        for k in ("J", "V", "s0", "b0", "w0", "fmin"):
            assert getattr(q, k) == g[f"{name}/out/{k}"].item(), (name, k)


def test_forward_inverse(golden):
    g = golden["cwt"]
    for name in sorted({k.split("/")[0] for k in g.files}):
        x = g[f"{name}/x"]
        f = abi.OracleFrame(int(g[f"{name}/type"]), int(g[f"{name}/J"]), int(g[f"{name}/V"]), len(x),
                            float(g[f"{name}/s0"]), float(g[f"{name}/b0"]), float(g[f"{name}/w0"]))
        Y = f.forward(x)
        assert Y.shape == g[f"{name}/Y"].shape
        assert abi.relerr(Y, g[f"{name}/Y"]) < TOL, name
        assert abi.relerr(f.inverse(g[f"{name}/Y"]), g[f"{name}/xrec"]) < TOL, name


def _case_input(g, name):
    tag = str(g[f"{name}/input"])
    return g["X"] if tag == "X" else g["Xodd"] if tag == "Xodd" else g[f"{name}/x"]


def _case_params(g, name):
    p = abi.t_tsPWS()
    for k in [k for k in g.files if k.startswith(f"{name}/in/")]:
        setattr(p, k.split("/")[-1], g[k].item())
    return p


def main_case_names(g):
    return sorted({k.split("/")[0] for k in g.files if "/in/" in k})


def check_main(fn, g, name, tol):
    p = _case_params(g, name)
    kw = dict(dt=float(g[f"{name}/dt"]), beg=float(g[f"{name}/beg"]))
    if f"{name}/times" in g.files:
        kw["times"] = g[f"{name}/times"]
    if f"{name}/reference" in g.files:
        kw["reference"] = g[f"{name}/reference"]
    abi.srand(1)  # random-subsampling masks come from libc rand()
    r = abi.run_main(fn, p, _case_input(g, name), **kw)
    assert r["rc"] == 0, name
    assert abi.relerr(r["ls"], g[f"{name}/ls"]) < tol, name
    assert abi.relerr(r["tsPWS"], g[f"{name}/tsPWS"]) < tol, name
    for k in ("J", "V", "s0", "b0", "w0", "fold"):
        assert getattr(r["params"], k) == g[f"{name}/out/{k}"].item(), (name, k)
    if f"{name}/sigall_after" in g.files:  # in-place mutation contract (fold / rm)
        assert abi.relerr(r["sigall"], g[f"{name}/sigall_after"]) < 1e-6, name
    if f"{name}/jk_ls" in g.files:
        np.testing.assert_array_equal(r["jk_mtr"], g[f"{name}/jk_mtr"])
        for c in range(len(r["jk_mtr"])):
            assert abi.relerr(r["jk_ls"][c], g[f"{name}/jk_ls"][c]) < tol, (name, c)
            assert abi.relerr(r["jk_ts"][c], g[f"{name}/jk_ts"][c]) < tol, (name, c)
    if f"{name}/sub_ls" in g.files:
        for c in range(g[f"{name}/sub_ls"].shape[0]):
            assert abi.relerr(r["sub_ls"][c], g[f"{name}/sub_ls"][c]) < tol, (name, c)
            assert abi.relerr(r["sub_ts"][c], g[f"{name}/sub_ts"][c]) < tol, (name, c)
    if f"{name}/conv_ls_sim" in g.files:
        # similarity curves are O(1); misfits are sums of squares of float-rounded references: compare relatively
        for k in ("ls_sim", "tsPWS_sim"):
            assert np.max(np.abs(r["conv_" + k] - g[f"{name}/conv_{k}"])) < 1e-9, (name, k)
        for k in ("ls_misfit", "tsPWS_misfit"):
            want = g[f"{name}/conv_{k}"]
            assert np.max(np.abs(r["conv_" + k] - want)) <= 1e-7 * np.max(np.abs(want)) + 1e-18, (name, k)
        if f"{name}/conv_ts_steps" in g.files:
            assert abi.relerr(r["conv_ts_steps"], g[f"{name}/conv_ts_steps"]) < tol, name
            assert abi.relerr(r["conv_ls_steps"], g[f"{name}/conv_ls_steps"]) < tol, name
    return r


def test_whole_calls(golden):
    g = golden["mains"]
    fn = abi.oracle().orc_tspws_main
    for name in main_case_names(g):
        check_main(fn, g, name, 2e-7)  # outputs are float32: one ulp of the peak


def test_example_data(golden):
    g = golden["example32"]
    fn = abi.oracle().orc_tspws_main
    for name in ("ex1", "ex2", "ex3", "ex_mexhat"):
        p = _case_params(g, name)
        r = abi.run_main(fn, p, g["traces"], dt=float(g["dt"]), beg=float(g["beg"]))
        assert abi.relerr(r["ls"], g[f"{name}/ls"]) < 2e-7, name
        assert abi.relerr(r["tsPWS"], g[f"{name}/tsPWS"]) < 2e-7, name
        assert r["params"].fold == g[f"{name}/out/fold"].item()


def test_parallel_restatement_is_bit_identical():
    """orc_tspws_main_mt (the stronger host baseline of bench.py) only redistributes loops."""
    X = abi.synth_traces(40, 4096, seed=5)
    for kw in (dict(Kmax=10, unbiased=1), dict(), dict(type=-3, Kmax=4), dict(wu=1.5)):
        p = abi.default_params(**kw)
        a = abi.run_main(abi.oracle().orc_tspws_main, p, X)
        b = abi.run_main(abi.oracle().orc_tspws_main_mt, p, X)
        np.testing.assert_array_equal(a["ls"], b["ls"])
        np.testing.assert_array_equal(a["tsPWS"], b["tsPWS"])


def test_empty_frame_returns_4_like_the_reference():
    """J resolved to 0 (fmin above the first scale): no scales -> CheckWaveletFamily fails (FWTa/wavelet_mem_v7.c:40-45), the
    coefficient containers are NULL and tspws_main returns 4 (ts_pws1f_lib.c:199-204), after fold / rm rewrote the traces.
    Known answer from the reference build: rc 4, outputs untouched; compared live when oracle/_ref is present."""
    kw = dict(type=-3, s0=4.823433067845736, fmin=0.04796741189352445, wu=1.5, Kmax=12, lrm=1)
    X = abi.synth_traces(9, 1000, seed=3) + np.float32(0.25)
    p = abi.default_params(**kw)
    b = abi.run_main(abi.oracle().orc_tspws_main, p, X)
    assert b["params"].J == 0 and b["rc"] == 4
    assert not b["ls"].any() and not b["tsPWS"].any()
    assert not np.array_equal(b["sigall"], X)   # the mean was removed before the failure
    ref = abi.ref()
    if ref is not None:
        r = abi.run_main(ref.tspws_main, p, X)
        assert r["rc"] == 4 and r["params"].J == 0
        np.testing.assert_array_equal(b["sigall"], r["sigall"])


def test_leap_day_jackknife_goldens(golden):
    """JackknifePlans' leap-day quirk (ts_pws1f_lib.c:398-401): tm_yday == 365 -- 31 December of a leap year -- falls into bin n,
    which no combination deletes, so such a trace is part of EVERY replica.  Reference goldens with two such traces."""
    g = golden["extra"]
    fn = abi.oracle().orc_tspws_main
    for name in main_case_names(g):
        check_main(fn, g, name, 2e-7)
    sizes = g["jk_leapday_n4_d1/jk_mtr"]
    assert sizes.min() >= 12 and sizes.sum() == 3 * 14 + 2 * 4  # 14 ordinary traces, each deleted from exactly one of the 4 replicas; the 2 leap-day traces from none
