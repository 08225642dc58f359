"""The refusals of tspws_hip_dtw_rows, through the C entry point on sentinel-filled outputs: TSPWS_E_ARG with the contract's message before
any device work, outputs untouched; the checks that need no plan come first (a NULL plan with bad parameters reports the parameters);
B == 0 or M == 0 returns 0 and does nothing; the binding raises the library's message."""
import ctypes as C
import importlib

import numpy as np
import pytest

import abi
import dtw_rows_ref as dr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N = dr.N
B, M = 2, 3


def test_refusals():
    import torch
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    plan = tspws.Plan(tspws.resolve(abi.default_params(), N), N)
    ranges = ((0, 1501), (700, 701))
    W, T = len(ranges), 1502
    d_rows = torch.ones((B, M, N + 3), dtype=torch.float32, device="cuda")
    d_ref = torch.ones((B, N + 1), dtype=torch.float32, device="cuda")
    o_fit = torch.full((B * M * W * 6,), -3.0, dtype=torch.float64, device="cuda")
    o_lag = torch.full((B * M * T,), 77, dtype=torch.int32, device="cuda")
    good = np.ascontiguousarray(np.array(ranges, dtype=np.uint64))

    def go(handle=plan.h, r=d_rows.data_ptr(), f=d_ref.data_ptr(), ld=N + 3, ldr=N + 1, nb=B, m=M, z=dr.Z, wa=good, nw=None, fit=True, nopar=False, Lmax=5, b=2):
        cp = tspws.dtw_par(Lmax, b)
        rc = lib.tspws_hip_dtw_rows(handle, r, ld, nb, m, None, f, ldr, z, None if nopar else C.addressof(cp), None if wa is None else wa.ctypes.data,
                                    (wa.shape[0] if wa is not None else 1) if nw is None else nw, o_lag.data_ptr(), o_fit.data_ptr() if fit else None, None)
        torch.cuda.synchronize()
        assert bool((o_fit == -3.0).all()) and bool((o_lag == 77).all())  # outputs untouched
        return rc, lib.tspws_hip_last_error()

    def win(*pairs):
        return np.ascontiguousarray(np.array(pairs, dtype=np.uint64))

    for bad in (dict(r=None), dict(f=None), dict(nopar=True), dict(wa=None), dict(fit=False), dict(handle=None)):
        assert go(**bad) == (-1, b"dtw_rows: NULL"), bad
    assert go(ld=N - 1) == (-1, b"dtw_rows: row stride below the trace length")
    assert go(ldr=N - 1) == (-1, b"dtw_rows: reference row stride below the trace length")
    for kw, msg in ((dict(Lmax=0), b"a largest lag outside [1, 127]"), (dict(Lmax=128), b"a largest lag outside [1, 127]"),
                    (dict(b=0), b"a strain limit outside [1, 8]"), (dict(b=9), b"a strain limit outside [1, 8]")):
        assert go(**kw) == (-1, b"dtw_rows: " + msg), kw
        assert go(handle=None, **kw) == (-1, b"dtw_rows: " + msg), kw      # judged before the plan is looked at
    assert go(nw=0) == (-1, b"dtw_rows: 1 to 4 lag ranges") and go(wa=win(*[(0, 9)] * 5)) == (-1, b"dtw_rows: 1 to 4 lag ranges")
    assert go(wa=win((0, 9), (700, 700))) == (-1, b"dtw_rows: an empty lag range (n0 >= n1)")
    assert go(wa=win((0, 9), (701, 700))) == (-1, b"dtw_rows: an empty lag range (n0 >= n1)")
    assert go(wa=win((0, 9), (5, 5 + 131073))) == (-1, b"dtw_rows: a lag range longer than 131072 samples")
    assert go(handle=None, wa=win((5, 5 + 131073))) == (-1, b"dtw_rows: a lag range longer than 131072 samples")
    assert go(wa=win((N - 3, N + 1))) == (-1, b"dtw_rows: a lag range past the trace length")
    assert go(z=float("nan")) == (-1, b"dtw_rows: a NaN or infinite zero-lag position") and go(z=float("inf"))[0] == -1 and go(z=float("-inf"))[0] == -1
    assert go(nb=0x10000, m=0x10000) == (-1, b"dtw_rows: more than 2^32 - 16 rows")
    assert go(nb=0)[0] == 0 and go(m=0)[0] == 0
    with pytest.raises(tspws.TspwsError, match="dtw_rows: a lag range past the trace length"):
        plan.dtw_rows(d_rows[:, :, :N], d_ref[:, :N], dr.Z, dict(Lmax=5, b=2), ((0, N + 1),))
    with pytest.raises(tspws.TspwsError, match="dtw_rows: a strain limit outside"):
        plan.dtw_rows(d_rows[:, :, :N], d_ref[:, :N], dr.Z, dict(Lmax=5, b=0), ranges)
    # the limits themselves pass: Lmax = 127, b = 8, W = 4 (constant rows: every lag ties, the first one wins everywhere)
    out = plan.dtw_rows(d_rows[:1, :1, :N], d_ref[:1, :N], dr.Z, dict(Lmax=127, b=8), ((0, N), (0, 1), (0, 1), (0, 1)))
    fit = out["fit"].cpu().numpy()
    assert fit[0, 0, 0, 4] == 0.0 and fit[0, 0, 0, 0] == 0.0 and fit[0, 0, 0, 5] == N and (out["lag"].cpu().numpy() == -127).all()
