"""GPU tests of the coherence filter (tspws_hip_filter_coef, tspws_hip_filter_traces), on the shipped library, against the checker
tests/filter_traces_ref.py.

The frames are the default Morlet at N = 2048 and at N = 1501 (D does not divide N: the seam) and the Mexican hat at N = 2048.  The batch is
B = 5 ensembles of 0, 1, 2, 3 and 70 traces (filter_traces_child.py); one trace is all zero.

1. filter_coef on the device's own Plan.forward bits with the checker's PS: every coefficient inside the bound (modes 0, 1 and 3; mode 2,
   wu = 1.5, inside the parity tolerance), loo 0 and 1, in place and out of place, ens given and NULL.
2. filter_coef bit for bit: repeated, in pieces against at once, a row alone against the row inside the batch.
3. filter_traces against the checker's rows from the same sets: single-stage biased and unbiased, two-stage Kmax = 4 (the 70 two-stage, the
   short ones single), loo = 1; per row max |diff| / max |row| <= 2e-6, NaN rows exactly where defined, repeated bit for bit.
4. The mean identity: per ensemble the float64 mean of the output rows against Plan.stack_batch's ts row, within
   2e-6 max |ts_b| + 2^-23 max_i max |x~_i| (the parity tolerance plus the float casts); single- and two-stage.
5. Row targets: M = 3 rows per ensemble from Plan.subsample_batch, counts of 0 giving NaN rows, against the checker.
6. A small budget in a child process: two rounds, one ensemble transformed twice, outputs within the tolerance of this process's."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_traces_child as fc
import filter_traces_ref as ftr
import inverse_rows_ref as irr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, T, COUNTS = fc.FIRST, fc.T, fc.COUNTS
ENS = np.repeat(np.arange(len(COUNTS)), COUNTS).astype(np.uint32)         # the ensemble of every trace
MODES = ((2.0, 0), (1.0, 0), (1.5, 0), (2.0, 1))                           # (wu, unbiased): modes 0, 1, 2, 3


@pytest.fixture(scope="module")
def torch():
    import torch
    assert tspws.load().tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def cases(torch):
    """Per frame: the plan, the checker's frame from it, the traces on the device and their device sets, downloaded once."""
    out = {}
    for name, (_, N) in fc.FRAMES.items():
        pl = fc.make_plan(name)
        X = fc.traces(N)
        d_X = torch.from_numpy(X).cuda()
        Y = pl.forward(d_X)
        hY = Y.cpu().numpy()
        assert np.isfinite(hY).all() and (hY[fc.ZERO] == 0).all()
        out[name] = dict(plan=pl, fr=irr.Frame.from_plan(pl), X=X, d_X=d_X, Y=Y, hY=hY, N=N)
    return out


def with_params(pl, wu=2.0, unbiased=0, Kmax=0):
    """The plan with these stack parameters (the frame does not depend on them)."""
    pl.params.wu, pl.params.unbiased, pl.params.Kmax = wu, unbiased, Kmax
    return pl


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("loo", (False, True))
@pytest.mark.parametrize("name", tuple(fc.FRAMES))
def test_filter_coef_against_the_checker(torch, cases, name, loo):
    c = cases[name]
    hY = c["hY"]
    # the ensembles with traces (leave-one-out: with two at least), renumbered 0 ..
    keep = [b for b, m in enumerate(COUNTS) if m >= (2 if loo else 1)]
    rows = np.concatenate([np.arange(FIRST[b], FIRST[b + 1]) for b in keep])
    ens = np.concatenate([np.full(COUNTS[b], j, np.uint32) for j, b in enumerate(keep)])
    K = np.array([COUNTS[b] for b in keep], np.uint32)
    PS = np.stack([ftr.phase_stack(hY[FIRST[b]:FIRST[b + 1]]).astype(np.complex128) for b in keep])
    d_PS = torch.from_numpy(PS).cuda()
    d_Y = c["Y"][torch.from_numpy(rows).cuda()].contiguous()
    for wu, unbiased in MODES:
        pl = with_params(c["plan"], wu, unbiased)
        got = pl.filter_coef(d_Y, d_PS, K, ens=ens, loo=loo)
        st = pl.filter_traces_stats()
        assert st["rows"] == len(rows) and st["rounds"] == 1, st
        h = got.cpu().numpy()
        modes = set()
        for j, b in enumerate(keep):
            sl = ens == j
            ref = ftr.reference(hY[rows[sl]], PS[j], int(K[j]), wu, unbiased, loo)
            modes.add(ref.mode)
            r = ftr.check_sets(h[sl], ref, f"{name} wu = {wu} unbiased = {unbiased} loo = {loo} ensemble of {COUNTS[b]}")
            print(name, "wu", wu, "unbiased", unbiased, "loo", loo, "M", COUNTS[b], "mode", ref.mode, "worst |diff| / bound", f"{r:.3g}")
        assert (h[rows == fc.ZERO] == 0).all()                     # the zero trace's set stays zero
        if unbiased:
            assert modes == {0, 3}                                  # K == 1 (leave-one-out: K - 1 == 1) falls back to the biased weight
        # in place: the same bits, and the input is the output
        Yc = d_Y.clone()
        assert pl.filter_coef(Yc, d_PS, K, ens=ens, loo=loo, out=Yc) is Yc and same(Yc.cpu().numpy(), h)
        assert same(d_Y.cpu().numpy(), hY[rows])                    # out of place leaves the input alone
        # without ens: one row per ensemble
        one = np.array([np.flatnonzero(ens == j)[-1] for j in range(len(keep))])
        alone = pl.filter_coef(d_Y[torch.from_numpy(one).cuda()].contiguous(), d_PS, K, loo=loo).cpu().numpy()
        assert same(alone, h[one])
    with_params(c["plan"])


@pytest.mark.parametrize("loo", (False, True))
def test_filter_coef_bit_identity(torch, cases, loo):
    c = cases["morlet1501"]
    pl = with_params(c["plan"], 2.0, 1)
    hY = c["hY"]
    lo = int(FIRST[2])                                              # ensembles 2, 3, 4 (2, 3 and 70 traces), renumbered
    ens = (ENS[lo:] - 2).astype(np.uint32)
    K = np.array(COUNTS[2:], np.uint32)
    d_PS = torch.from_numpy(np.stack([ftr.phase_stack(hY[FIRST[b]:FIRST[b + 1]]).astype(np.complex128) for b in (2, 3, 4)])).cuda()
    d_Y = c["Y"][lo:].contiguous()
    full = pl.filter_coef(d_Y, d_PS, K, ens=ens, loo=loo).cpu().numpy()
    assert np.isfinite(full).all()
    assert same(pl.filter_coef(d_Y, d_PS, K, ens=ens, loo=loo).cpu().numpy(), full)          # repeated
    cut = 29                                                                                    # inside the 70, inside a slab
    parts = [pl.filter_coef(d_Y[a:e].contiguous(), d_PS, K, ens=ens[a:e], loo=loo).cpu().numpy() for a, e in ((0, cut), (cut, len(ens)))]
    assert same(np.concatenate(parts), full)                                                    # in pieces against at once
    for i in (0, 3, 40, len(ens) - 1):                                                          # a row alone against the row inside the batch
        assert same(pl.filter_coef(d_Y[i:i + 1].contiguous(), d_PS, K, ens=ens[i:i + 1], loo=loo).cpu().numpy(), full[i:i + 1]), i
    with_params(pl)


TRACE_CASES = {
    "morlet2048": (("biased", 2.0, 0, 0, False), ("unbiased", 2.0, 1, 0, False), ("two_stage_K4", 2.0, 1, 4, False), ("loo", 2.0, 1, 0, True)),
    "morlet1501": (("biased", 2.0, 0, 0, False), ("loo", 2.0, 0, 0, True)),
    "mexhat2048": (("unbiased", 2.0, 1, 0, False),),
}


@pytest.mark.parametrize("name,case", [(n, k) for n, ks in TRACE_CASES.items() for k in ks], ids=lambda v: v if isinstance(v, str) else v[0])
def test_filter_traces_against_the_checker(torch, cases, name, case):
    what, wu, unbiased, Kmax, loo = case
    c = cases[name]
    pl = with_params(c["plan"], wu, unbiased, Kmax)
    got = pl.filter_traces(c["d_X"], FIRST, loo=loo)
    st = pl.filter_traces_stats()
    h = got.cpu().numpy()
    assert h.shape == (T, c["N"]) and h.dtype == np.float32
    want = fc.want_rows(c["fr"], c["hY"], FIRST, wu, unbiased, Kmax, loo)
    worst = fc.check_rows(h, want, f"{name} {what}")
    print(name, what, "worst max |diff| / max |row| =", f"{worst:.3g}", st)
    left = 1 if loo else 0                                          # leave-one-out leaves the one-trace ensemble out
    assert st == dict(rounds=1, rows=T - left, left_out=left, single_stage=3 if Kmax else 4, two_stage=1 if Kmax else 0, empty=1, twice=0), st
    assert np.isnan(h[0]).all() == bool(loo) and (h[fc.ZERO] == 0).all()
    assert same(pl.filter_traces(c["d_X"], FIRST, loo=loo).cpu().numpy(), h)                   # repeated
    assert same(c["d_X"].cpu().numpy(), c["X"])                                                 # the traces are unchanged
    with_params(pl)


@pytest.mark.parametrize("Kmax", (0, 4))
@pytest.mark.parametrize("unbiased", (0, 1))
@pytest.mark.parametrize("name", ("morlet2048", "morlet1501"))
def test_mean_of_the_filtered_traces_is_the_stack(torch, cases, name, unbiased, Kmax):
    c = cases[name]
    pl = with_params(c["plan"], 2.0, unbiased, Kmax)
    x = pl.filter_traces(c["d_X"], FIRST).cpu().numpy().astype(np.float64)
    _, ts = pl.stack_batch(c["d_X"], FIRST)
    torch.cuda.synchronize()
    ts = ts.cpu().numpy().astype(np.float64)
    for b, m in enumerate(COUNTS):
        if not m:
            continue
        rows = x[FIRST[b]:FIRST[b + 1]]
        mean = rows.sum(axis=0) / m
        lim = 2e-6 * np.abs(ts[b]).max() + 2.0 ** -23 * np.abs(rows).max()
        err = np.abs(mean - ts[b]).max()
        print(name, "unbiased", unbiased, "Kmax", Kmax, "M", m, "max |mean - ts| =", f"{err:.3g}", "limit", f"{lim:.3g}")
        assert err <= lim, (name, unbiased, Kmax, m, err, lim)
    with_params(pl)


def test_row_targets(torch, cases):
    c = cases["morlet2048"]
    N = c["N"]
    pl = with_params(c["plan"], 2.0, 1)
    sel = np.ones((3, T), np.int8)
    sel[1, ::2] = 0              # every other trace: the one-trace ensemble keeps nothing in row 1
    sel[2, :5] = 0
    sel[2, 40:] = 0              # row 2: nothing of the ensembles of 1 and 2 traces
    _, ts_out, mtr = pl.subsample_batch(c["d_X"], FIRST, sel)
    torch.cuda.synchronize()
    assert mtr.shape == (5, 3) and (mtr[0] == 0).all() and mtr[1, 1] == 0 and mtr[1, 2] == 0 and mtr[2, 2] == 0 and (mtr[3:] > 0).all()
    got = pl.filter_traces(c["d_X"], FIRST, rows=ts_out, mtr=mtr)
    st = pl.filter_traces_stats()
    left = int((mtr == 0).sum())
    assert left == 6 and st == dict(rounds=1, rows=15 - left, left_out=left, single_stage=4, two_stage=0, empty=1, twice=0), st
    h = got.cpu().numpy()
    assert h.shape == (5, 3, N)
    # the checker: the rows' own sets with the W of the ensemble's traces
    hR = pl.forward(ts_out.view(15, N)).cpu().numpy()
    want = np.full((5, 3, N), np.nan)
    for b, m in enumerate(COUNTS):
        take = np.flatnonzero(mtr[b] > 0)
        if not m or not take.size:
            continue
        PS = ftr.phase_stack(c["hY"][FIRST[b]:FIRST[b + 1]]).astype(np.complex128)
        ref = ftr.reference(hR[3 * b + take], PS, m, 2.0, 1)
        want[b, take] = ftr.rows_of(c["fr"], ref.want).astype(np.float64)
    worst = fc.check_rows(h.reshape(15, N), want.reshape(15, N), "row targets")
    print("row targets: worst max |diff| / max |row| =", f"{worst:.3g}")
    # without counts every row of an ensemble with traces takes part
    every = pl.filter_traces(c["d_X"], FIRST, rows=ts_out).cpu().numpy()
    assert pl.filter_traces_stats()["left_out"] == 3 and np.isnan(every[0]).all() and np.isfinite(every[1:]).all()
    assert same(every[mtr > 0], h[mtr > 0])
    with_params(pl)


def test_small_budget_takes_rounds_and_transforms_twice(torch, tmp_path):
    """The budget batch under TSPWS_PART_MB=16 in a child process (two rounds, the 150-trace ensemble transformed twice) against the one-round
    outputs of this process."""
    o0, s0, o1, s1 = fc.run_budget(torch)
    assert s0["rounds"] == 1 and s0["twice"] == 0 and s0["rows"] == T + fc.BIG and s1["rows"] == T + fc.BIG - 1, (s0, s1)
    path = str(tmp_path / "small.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "filter_traces_child.py"), path], capture_output=True, text=True,
                         env=dict(os.environ, TSPWS_PART_MB="16"), timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "FILTER_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    small = np.load(path)
    assert (small["rounds"] > 1).all() and (small["twice"] == 1).all(), (small["rounds"], small["twice"])
    assert small["rows"].tolist() == [s0["rows"], s1["rows"]]
    for key, mine in (("o0", o0), ("o1", o1)):
        worst = fc.check_rows(small[key], mine.astype(np.float64), "small budget " + key)
        print("small budget", key, "worst max |diff| / max |row| =", f"{worst:.3g}")
