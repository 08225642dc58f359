"""The refusals of tspws_hip_mwcs_rows, through the C entry point on sentinel-filled outputs: TSPWS_E_ARG with the contract's message
before any device work, outputs untouched; the checks that need no plan come first (a NULL plan with bad parameters reports the
parameters); B == 0 or M == 0 returns 0 and does nothing; the binding raises the library's message."""
import ctypes as C
import importlib

import numpy as np
import pytest

import abi
import mwcs_rows_ref as mr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N = mr.N
B, M = 2, 6


def test_refusals():
    import torch
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    plan = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    par, ranges = mr.SETS["i"]
    W, J, Qx = len(ranges), len(mr.windows(par, ranges)), par.Qx
    rows, ref, _ = mr.parity_batch(3, B, M)
    d_rows, d_ref = torch.from_numpy(rows).cuda(), torch.from_numpy(ref).cuda()
    outs = [torch.full((n,), -3.0, dtype=torch.float64, device="cuda") for n in (B * M * J * 3, B * M * W * 6, B * M * J * Qx * 2, B * J * Qx * 2)]
    good = np.ascontiguousarray(np.array(ranges, dtype=np.uint64))

    def go(handle=plan.h, r=d_rows.data_ptr(), f=d_ref.data_ptr(), ld=N + 3, ldr=N + 1, nb=B, m=M, z=mr.Z, wa=good, nw=None, fit=True, nopar=False, **kw):
        cp = tspws.mwcs_par(**dict(par.kwargs(), **kw))
        rc = lib.tspws_hip_mwcs_rows(handle, r, ld, nb, m, None, f, ldr, z, None if nopar else C.addressof(cp), None if wa is None else wa.ctypes.data,
                                     (wa.shape[0] if wa is not None else 1) if nw is None else nw, outs[0].data_ptr(), outs[1].data_ptr() if fit else None,
                                     outs[2].data_ptr(), outs[3].data_ptr(), None)
        torch.cuda.synchronize()
        assert all(bool((o == -3.0).all()) for o in outs)  # outputs untouched
        return rc, lib.tspws_hip_last_error()

    def win(*pairs):
        return np.ascontiguousarray(np.array(pairs, dtype=np.uint64))

    for bad in (dict(r=None), dict(f=None), dict(nopar=True), dict(wa=None), dict(fit=False), dict(handle=None)):
        assert go(**bad) == (-1, b"mwcs_rows: NULL"), bad
    assert go(ld=N - 1) == (-1, b"mwcs_rows: row stride below the trace length")
    assert go(ldr=N - 1) == (-1, b"mwcs_rows: reference row stride below the trace length")
    for kw, msg in ((dict(L=15), b"a window length outside [16, 1024]"), (dict(L=1025, P=2048), b"a window length outside [16, 1024]"),
                    (dict(hop=0), b"a hop outside [1, L]"), (dict(hop=101), b"a hop outside [1, L]"),
                    (dict(P=64), b"a DFT length that is no power of two in [L, 4096]"), (dict(P=192), b"a DFT length that is no power of two in [L, 4096]"),
                    (dict(P=8192), b"a DFT length that is no power of two in [L, 4096]"),
                    (dict(q0=0), b"a band outside 1 <= q0, q0 + 2 <= q1 <= P / 2"), (dict(q0=19), b"a band outside 1 <= q0, q0 + 2 <= q1 <= P / 2"),
                    (dict(q1=65), b"a band outside 1 <= q0, q0 + 2 <= q1 <= P / 2"), (dict(h=9), b"a smoothing half-width above 8"),
                    (dict(taper=1.5), b"a taper fraction outside [0, 1]"), (dict(taper=float("nan")), b"a taper fraction outside [0, 1]"),
                    (dict(min_coh=float("nan")), b"a NaN filter"), (dict(err_floor=0.0), b"an error floor that is not positive and finite"),
                    (dict(q0=1, q1=64, h=1), b"more than 64 bins with the smoothing margins")):
        assert go(**kw) == (-1, b"mwcs_rows: " + msg), kw
        assert go(handle=None, **kw) == (-1, b"mwcs_rows: " + msg), kw      # judged before the plan is looked at
    assert go(nw=0) == (-1, b"mwcs_rows: 1 to 4 lag ranges") and go(wa=win(*[(0, N)] * 5)) == (-1, b"mwcs_rows: 1 to 4 lag ranges")
    assert go(wa=win((0, N), (700, 700))) == (-1, b"mwcs_rows: an empty lag range (n0 >= n1)")
    assert go(wa=win((0, N + 1))) == (-1, b"mwcs_rows: a lag range past the trace length")
    assert go(z=float("nan")) == (-1, b"mwcs_rows: a NaN or infinite zero-lag position") and go(z=float("inf"))[0] == -1
    assert go(wa=win((700, 712), (3, 99))) == (-1, b"mwcs_rows: no lag range holds a window")
    assert go(wa=win(*[(0, N)] * 4), L=16, hop=1, P=16, q0=1, q1=3) == (-1, b"mwcs_rows: more than 4096 windows")
    assert go(nb=0x10000, m=0x10000) == (-1, b"mwcs_rows: more than 2^32 - 16 rows")
    assert go(nb=0)[0] == 0 and go(m=0)[0] == 0
    with pytest.raises(tspws.TspwsError, match="mwcs_rows: a lag range past the trace length"):
        plan.mwcs_rows(d_rows[:, :, :N], d_ref[:, :N], mr.Z, par.kwargs(), ((0, N + 1),))
    with pytest.raises(tspws.TspwsError, match="mwcs_rows: a hop outside"):
        plan.mwcs_rows(d_rows[:, :, :N], d_ref[:, :N], mr.Z, dict(par.kwargs(), hop=0), ranges)
