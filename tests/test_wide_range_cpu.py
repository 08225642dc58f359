"""Pin the oracle against the reference itself on a wide-dynamic-range ensemble (tests/golden/ref_wide256.npz, written by
`make_golden.py wide`): spikes over backgrounds 8 .. 40 decades below them, exact zeros and float subnormals among ordinary traces.  The
reference counts the phasor of every coefficient except an exact 0 / 0 (ts_pws1f_lib.c:486-494); the oracle must do the same on the quiet
parts of these traces, where the phase stack is most sensitive.  CPU only; the inputs are rebuilt from the stored seed."""
import os

import numpy as np

import abi

HERE = os.path.dirname(os.path.abspath(__file__))


def wide_fixture():
    g = np.load(os.path.join(HERE, "golden", "ref_wide256.npz"), allow_pickle=False)
    X = abi.wide_traces(int(g["mtr"]), int(g["N"]), seed=int(g["seed"]), every=int(g["every"]))
    return g, X


WIDE_CASES = (("morlet", dict()), ("exact_morlet_wu15", dict(type=-2, wu=1.5)), ("mexhat", dict(type=-3)))


def test_wide_ensemble_has_the_intended_traces():
    _, X = wide_fixture()
    rows = X[::19][:12]
    peak = np.abs(rows).max(axis=1)
    quiet = np.array([np.abs(r[np.abs(r) < 0.5 * p]).max() if p else 0.0 for r, p in zip(rows, peak)])
    assert (peak[:8] == 1.0).all() and peak[9] == 1.0 and peak[10] < 1e-39 and 0 < peak[11] < 1e-29
    assert quiet[7] == 0.0                                     # spike over an exact zero
    assert (rows[8][:2048] == 0).all() and 0 < np.sort(np.abs(rows[8]))[-129] <= 1e-13   # half zero, half 1e-13, one unit segment
    assert 1e-41 < quiet[9] <= 1e-40 and (rows[10] != 0).sum() > 1000   # float subnormals
    for b, q in zip(abi.WIDE_BACKGROUNDS, quiet[:7]):
        assert 0.5 * b < q <= b, (b, q)


def test_oracle_vs_reference_on_wide_ensemble():
    g, X = wide_fixture()
    for name, kw in WIDE_CASES:
        r = abi.run_main(abi.oracle().orc_tspws_main, abi.default_params(**kw), X)
        assert r["rc"] == 0, name
        assert abi.relerr(r["ls"], g[f"{name}/ls"]) < 2e-7, name     # outputs are float32: one ulp of the peak
        assert abi.relerr(r["tsPWS"], g[f"{name}/tsPWS"]) < 2e-7, name
