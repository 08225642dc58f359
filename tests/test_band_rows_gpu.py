"""The band rows of the inverse (tspws_hip_inverse_bands, Plan.inverse_bands) on the GPU, held to the CPU reference of tests/band_rows_ref.py
at EVERY sample of every row: frames and seeds of tests/inverse_rows_engine.CASES (the smallest frame that reaches each body of k_inv_poly),
one table per frame -- every single scale, [0, S), an empty band, two overlapping bands that cut octaves between voices, the last scale alone --
in ONE call, with 1, 2 and 5 sets, with and without the quadrature.  Then what needs no tolerance: a repeated call, a band alone in a table
of its own, a set alone in a call of its own, the real rows with and without the quadrature, the quadrature against the real rows of the
rotated set; and [0, S) against Plan.inverse within the sum of the two bounds.  The worst ratios go to TSPWS_BAND_REPORT when it is set."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import band_rows_ref as brr
import abi

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
CASES = brr.gpu_cases()


@pytest.fixture(scope="module")
def lib():
    lib = tspws.load()
    assert lib.tspws_hip_device_count() > 0, "no MI355X visible: the HIP path cannot run (there is no CPU fallback)"
    return lib


def report(line):
    print(line, flush=True)
    path = os.environ.get("TSPWS_BAND_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


@pytest.mark.parametrize("c,counts", CASES, ids=[brr.case_id(c) for c, _ in CASES])
def test_band_rows(lib, c, counts):
    N = c["N"]
    pl = tspws.Plan(tspws.resolve(abi.default_params(**c["kw"]), N), N)
    fr = brr.Frame.from_plan(pl)
    info = pl.inverse_info()
    nmax = max(counts)
    Y = brr.band_sets(c, fr, nmax)
    table = brr.band_table(fr.S, fr.V)
    ref = brr.reference_bands(fr, Y, table)
    assert ref.cap_ratio < brr.CAP
    worst = {}
    full = table.index((0, fr.S))
    X5 = Q5 = None
    for n in counts:
        X, Q = pl.inverse_bands(Y[:n], table, quadrature=True)
        X0 = pl.inverse_bands(Y[:n], table)
        worst[(n, "re")] = brr.check_bands(X, ref, 0)
        worst[(n, "im")] = brr.check_bands(Q, ref, 1)
        worst[(n, "re, no quadrature")] = brr.check_bands(X0, ref, 0)
        assert X0.tobytes() == X.tobytes(), (n, "real rows with and without the quadrature")
        X2, Q2 = pl.inverse_bands(Y[:n], table, quadrature=True)
        assert X2.tobytes() == X.tobytes() and Q2.tobytes() == Q.tobytes(), (n, "a repeated call")
        assert not X[:, table.index((min(3, fr.S), min(3, fr.S)))].any() and not Q[:, table.index((min(3, fr.S), min(3, fr.S)))].any(), "an empty band"
        # the quadrature of Y is the real row of -i Y: the same chain of operations on the rotated set
        assert pl.inverse_bands(brr.rotate(Y[:n]), table).tobytes() == Q.tobytes(), (n, "quadrature against the real rows of the rotated sets")
        # [0, S) against the existing inverse: both within their bound of the same reference row (a sum over all S scales: the same bound)
        xi = pl.inverse(Y[:n])
        both = 2 * ref.bound[0][:n, full]
        diff = np.abs(X[:, full].astype(brr.LD) - xi.astype(brr.LD))
        assert np.isfinite(xi).all() and (diff <= both).all(), (n, "[0, S) against Plan.inverse", float((diff / both).max()))
        worst[(n, "[0, S) against Plan.inverse")] = float((diff / both).max())
        if n == nmax:
            X5, Q5 = X, Q
    # the row of a band does not depend on the other bands of the table: every band alone in a table of its own
    for r, b in enumerate(table):
        Xa, Qa = pl.inverse_bands(Y, [b], quadrature=True)
        assert Xa[:, 0].tobytes() == X5[:, r].tobytes() and Qa[:, 0].tobytes() == Q5[:, r].tobytes(), ("band alone", r, b)
    Xa = pl.inverse_bands(Y, [table[-1], table[fr.S + 2]])  # (no quadrature: pairs of sets)
    assert Xa[:, 0].tobytes() == X5[:, -1].tobytes() and Xa[:, 1].tobytes() == X5[:, fr.S + 2].tobytes(), "bands alone, real rows only"
    # ... nor on the other sets of the call
    for j in range(nmax):
        Xj, Qj = pl.inverse_bands(Y[j: j + 1], table, quadrature=True)
        assert Xj[0].tobytes() == X5[j].tobytes() and Qj[0].tobytes() == Q5[j].tobytes(), ("set alone", j)
        assert pl.inverse_bands(Y[j: j + 1], table)[0].tobytes() == X5[j].tobytes(), ("set alone, real rows only", j)
    assert pl.inverse_info() == info  # the list tspws_hip_inverse launches is as it was
    w = max(worst.values())
    assert w <= 1
    report(f"BAND_ROWS {brr.case_id(c)}: S = {fr.S}, {len(table)} bands, sets {counts} | cap ratio {ref.cap_ratio:.2e} | worst |diff| / bound {w:.3g} ("
           + ", ".join(f"{k[0]} set(s) {k[1]} {v:.3g}" for k, v in sorted(worst.items(), key=lambda kv: str(kv[0]))) + ") | repeated call, band alone, "
           "set alone, with / without quadrature, rotated set: bit-identical")


def test_refusals(lib):
    """What needs the plan's S; the other refusals are in tests/test_band_rows_cpu.py."""
    import torch
    N = 64
    pl = tspws.Plan(tspws.resolve(abi.default_params(J=2), N), N)
    Y = torch.zeros((2, pl.ncoef), dtype=torch.complex128, device="cuda")
    out = torch.full((2, 2, N), 7.0, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for t in ([(0, pl.S + 1), (0, 1)], [(0, 1), (pl.S + 1, pl.S + 1)]):
        bt = tspws.band_table(t)
        assert lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), 2, bt.ctypes.data, 2, out.data_ptr(), out.data_ptr(), st) == -1
        assert b"inverse_bands: a band ends behind the last scale" in lib.tspws_hip_last_error()
    bt = tspws.band_table([(0, 1), (1, 2)])
    assert lib.tspws_hip_inverse_bands(pl.h, None, 2, bt.ctypes.data, 2, out.data_ptr(), None, st) == -1
    assert lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), 2, bt.ctypes.data, 2, None, None, st) == -1
    assert lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), 2, None, 2, out.data_ptr(), None, st) == -1
    # R = 0 and nset = 0: nothing to do
    assert lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), 2, bt.ctypes.data, 0, out.data_ptr(), None, st) == 0
    assert lib.tspws_hip_inverse_bands(pl.h, Y.data_ptr(), 0, bt.ctypes.data, 2, out.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(tspws.TspwsError):
        pl.inverse_bands(np.zeros((1, pl.ncoef), np.complex128), [(2, 1)])
    # a table of empty bands only: zero rows, no scale with a work item
    X, Q = pl.inverse_bands(np.ones((3, pl.ncoef), np.complex128), [(0, 0), (pl.S, pl.S)], quadrature=True)
    assert X.shape == (3, 2, N) and not X.any() and not Q.any()
