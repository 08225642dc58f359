"""What the coherence filter refuses (tspws_hip_filter_traces, tspws_hip_filter_coef), through the C entry points on NaN-filled outputs: every
refusal returns TSPWS_E_ARG with its message, before any device work and with the outputs untouched; B = 0 and empty inputs do nothing; and
the binding's own checks."""
import ctypes as C
import importlib

import numpy as np
import pytest

import abi
import filter_traces_child as fc

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N = 1501
FIRST = fc.FIRST
T = fc.T


@pytest.fixture(scope="module")
def torch():
    import torch
    assert tspws.load().tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def plan(torch):
    return fc.make_plan("morlet1501")


def test_filter_traces_refusals(torch, plan):
    lib = plan.lib
    d_X = torch.from_numpy(fc.traces(N)).cuda()
    rows = torch.zeros((5, 3, N), dtype=torch.float32, device="cuda")
    out = torch.full((T, N), float("nan"), dtype=torch.float32, device="cuda")
    f = np.ascontiguousarray(FIRST, dtype=np.uint64)
    mtr = np.ones((5, 3), np.uint32)
    two = tspws.t_tsPWS.from_buffer_copy(plan.params)
    two.Kmax = 4

    def call(h=plan.h, p=plan.params, x=d_X.data_ptr(), ld=N, first=f, B=5, r=None, ldr=0, M=0, m=None, loo=0, o=out.data_ptr(), ldo=N):
        rc = lib.tspws_hip_filter_traces(h, C.byref(p) if p is not None else None, x, ld, first.ctypes.data if first is not None else None, B, r, ldr, M,
                                         m.ctypes.data if m is not None else None, loo, o, ldo, None)
        msg = lib.tspws_hip_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())         # outputs untouched
        return rc, msg

    dec = f.copy()
    dec[2], dec[3] = dec[3], dec[2]
    R = rows.data_ptr()
    for kw, text in ((dict(p=None), b"NULL"), (dict(first=None), b"NULL"), (dict(o=None), b"NULL"), (dict(x=None), b"NULL"), (dict(h=None), b"NULL"),
                     (dict(first=dec), b"decreasing ensemble offsets"),
                     (dict(loo=2), b"loo must be 0 or 1"), (dict(loo=-1), b"loo must be 0 or 1"),
                     (dict(r=R, ldr=N, M=0), b"target rows without M"),
                     (dict(M=3), b"M or counts without target rows"), (dict(m=mtr), b"M or counts without target rows"),
                     (dict(r=R, ldr=N, M=3, loo=1), b"leave-one-out takes the ensembles' own traces, not target rows"),
                     (dict(p=two, loo=1), b"leave-one-out with a two-stage ensemble"),
                     (dict(ld=N - 1), b"row stride below the trace length"), (dict(ldo=N - 1), b"row stride below the trace length"),
                     (dict(r=R, ldr=N - 1, M=3), b"row stride below the trace length")):
        assert call(**kw) == (-1, b"filter_traces: " + text), kw
    # what needs no plan is refused without one, too, and first
    assert call(h=None, loo=2) == (-1, b"filter_traces: loo must be 0 or 1")
    assert call(h=None, first=dec, ld=1) == (-1, b"filter_traces: decreasing ensemble offsets")
    # B == 0 returns 0 and does nothing
    assert call(B=0)[0] == 0
    # ensembles without traces write nothing with trace targets
    assert call(first=np.full(6, 7, np.uint64))[0] == 0
    # the call itself works on this output
    rc =lib.tspws_hip_filter_traces(plan.h, C.byref(plan.params), d_X.data_ptr(), N, f.ctypes.data, 5, None, 0, 0, None, 0, out.data_ptr(), N, None)
    assert rc == 0 and bool(torch.isfinite(out).all())

    # the binding's own checks
    with pytest.raises(tspws.TspwsError, match="mtr needs rows"):
        plan.filter_traces(d_X, FIRST, mtr=mtr)
    with pytest.raises(tspws.TspwsError, match="rows must hold the B = 5 ensembles"):
        plan.filter_traces(d_X, FIRST, rows=rows[:4])
    with pytest.raises(tspws.TspwsError, match="first must be non-decreasing"):
        plan.filter_traces(d_X, dec.astype(np.int64))
    with pytest.raises(tspws.TspwsError, match="out must be"):
        plan.filter_traces(d_X, FIRST, out=torch.zeros((T, N + 1), dtype=torch.float32, device="cuda"))
    with pytest.raises(tspws.TspwsError, match="filter_traces: leave-one-out takes"):
        plan.filter_traces(d_X, FIRST, rows=rows, loo=True)
    assert tuple(plan.filter_traces(d_X, FIRST[:1]).shape) == (0, N)
    # new outputs hold NaN where nothing is written: trace targets of empty ensembles write nothing
    empty = plan.filter_traces(d_X, np.array([3, 3, 3]))
    assert tuple(empty.shape) == (0, N)


def test_filter_coef_refusals(torch, plan):
    lib = plan.lib
    nc = plan.ncoef
    Y = torch.full((4, nc), complex(1.0, -1.0), dtype=torch.complex128, device="cuda")
    PS = torch.full((2, nc), complex(0.5, 0.5), dtype=torch.complex128, device="cuda")
    out = torch.full((4, nc), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    K = np.array([3, 2], np.uint32)
    ens = np.array([0, 0, 1, 1], np.uint32)

    def call(h=plan.h, y=Y.data_ptr(), e=ens, nrow=4, ps=PS.data_ptr(), k=K, B=2, wu=2.0, loo=0):
        rc = lib.tspws_hip_filter_coef(h, y, e.ctypes.data if e is not None else None, nrow, ps, k.ctypes.data if k is not None else None, B, wu, 0, loo,
                                       out.data_ptr(), None)
        msg = lib.tspws_hip_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(torch.view_as_real(out)).all())      # outputs untouched
        return rc, msg

    for kw, text in ((dict(y=None), b"NULL"), (dict(ps=None), b"NULL"), (dict(k=None), b"NULL"), (dict(h=None), b"NULL"),
                     (dict(loo=3), b"loo must be 0 or 1"), (dict(wu=float("nan")), b"a NaN or infinite power"),
                     (dict(k=np.array([3, 0], np.uint32)), b"a count of 0"),
                     (dict(k=np.array([3, 1], np.uint32), loo=1), b"leave-one-out needs counts >= 2"),
                     (dict(e=np.array([0, 0, 1, 2], np.uint32)), b"an ensemble index >= B"),
                     (dict(e=None), b"without h_ens the rows must number B"),
                     (dict(nrow=0xfffffff1), b"more than 2^32 - 16 rows")):
        assert call(**kw) == (-1, b"filter_coef: " + text), kw
    assert call(nrow=0)[0] == 0 and call(B=0, k=K)[0] == 0
    with pytest.raises(tspws.TspwsError, match="without ens"):
        plan.filter_coef(Y, PS, K)
    with pytest.raises(tspws.TspwsError, match="K must be"):
        plan.filter_coef(Y, PS, K[:1], ens=ens)
    with pytest.raises(tspws.TspwsError, match="out must be"):
        plan.filter_coef(Y, PS, K, ens=ens, out=out[:3])
    got = plan.filter_coef(Y, PS, K, ens=ens, out=out)
    assert got is out and bool(torch.isfinite(torch.view_as_real(out)).all())
