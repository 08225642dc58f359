"""The checker of the coherence filter (tests/filter_traces_ref.py) tested on the CPU: the weight of hand cases, the leave-one-out weight
against the ensemble weight of the ensemble without the trace, the skip rule, the mean identity against the reference's tsPWS on the
16 x 2048 golden (single-stage, biased and unbiased) inside the project's parity tolerance, the checker's own verdicts, and the host plan
(csrc/filter_plan.h) against a direct enumeration as a stand-alone program under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import abi
import filter_traces_ref as ftr
import inverse_rows_ref as irr
from test_oracle_vs_golden import _case_input, _case_params

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_hand_cases():
    for K in (2, 3, 7, 70):
        PS = np.array([K, -K, 1j * K, K / np.sqrt(2) * (1 + 1j), 0, 1], np.complex128)
        for mode, wu in ((0, 2.0), (1, 1.0), (2, 1.5), (3, 2.0)):
            W, mag = ftr.weight(PS, K, mode, wu)
            assert np.abs(W[:4] - 1).max() < 1e-15, (K, mode, W)      # PS = K (full coherence) gives 1 in every mode
            assert (mag >= np.abs(W)).all()
            if mode != 3:
                assert W[4] == 0
        # mode 3 is negative below c = 1 / K, zero at it, -1 / (K - 1) at PS = 0
        W, _ = ftr.weight(np.array([0, np.sqrt(K) * 0.99, np.sqrt(K), np.sqrt(K) * 1.01], np.complex128), K, 3, 2.0)
        assert W[0] == -1 / LD(K - 1) and W[1] < 0 and abs(W[2]) < 1e-15 and W[3] > 0
    assert [ftr.weight_mode(*a) for a in ((2, 0, 5), (2, 1, 5), (2, 1, 1), (1, 1, 5), (1.5, 0, 5), (2, 1, 2))] == [0, 3, 0, 1, 2, 3]


def _sets(M, n, seed):
    rng = np.random.default_rng(seed)
    Y = (rng.standard_normal((M, n)) + 1j * rng.standard_normal((M, n))).astype(np.complex128)
    Y[:, :8] *= np.exp(-1j * np.angle(Y[:, :8]))     # a coherent stretch
    return Y


@pytest.mark.parametrize("wu,unbiased", ((2.0, 0), (2.0, 1), (1.0, 0), (1.5, 0)))
def test_loo_is_the_ensemble_without_the_trace(wu, unbiased):
    for M in (2, 3, 9):
        Y = _sets(M, 64, M)
        Y[1, 5] = 0          # skipped by the rule: nothing to subtract
        Y[0, 9:12] = 0
        PS = ftr.phase_stack(Y).astype(np.complex128)
        loo = ftr.reference(Y, PS, M, wu, unbiased, loo=True)
        assert loo.K == M - 1 and loo.mode == ftr.weight_mode(wu, unbiased, M - 1)
        if M == 2:
            assert loo.mode in (0, 1, 2)      # K - 1 == 1 falls back to the biased weight
        for i in range(M):
            rest = np.delete(Y, i, axis=0)
            PSr = ftr.phase_stack(rest)
            Wr, _ = ftr.weight(PSr, M - 1, loo.mode, wu)
            scale = np.maximum(np.abs(Wr), 1)
            assert (np.abs(loo.W[i] - Wr) <= 1e-14 * scale).all(), (M, i)
        # the zero coefficient's phasor is not subtracted: its weight is the full PS's
        Wfull, _ = ftr.weight(PS, M - 1, loo.mode, wu)
        assert loo.W[1, 5] == Wfull[5]


def test_skip_rule_and_zero_trace():
    Y = _sets(5, 32, 3)
    Y[2] = 0
    PS = ftr.phase_stack(Y)
    assert np.abs(PS - ftr.phase_stack(np.delete(Y, 2, axis=0))).max() == 0
    ref = ftr.reference(Y, PS.astype(np.complex128), 5, 2.0, 0)
    assert (ref.want[2] == 0).all() and (ref.bound[2] == 0).all()
    # the checker's verdicts: exact passes, one wrong coefficient fails with its place, NaN fails
    good = ref.want.astype(np.complex128)
    assert ftr.check_sets(good, ref) <= 1.0
    bad = good.copy()
    bad[3, 17] *= 1 + 1e-12
    with pytest.raises(ftr.FilterMismatch) as e:
        ftr.check_sets(bad, ref)
    assert (e.value.row, e.value.index) == (3, 17)
    bad = good.copy()
    bad[2, 4] = 1e-300      # the zero trace's set must stay exactly zero
    with pytest.raises(ftr.FilterMismatch):
        ftr.check_sets(bad, ref)
    bad = good.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ftr.FilterMismatch):
        ftr.check_sets(bad, ref)
    # a wrong K is far outside
    with pytest.raises(ftr.FilterMismatch):
        ftr.check_sets(ftr.reference(Y, PS.astype(np.complex128), 4, 2.0, 0).want.astype(np.complex128), ref)
    # mode 2 is held to the parity tolerance
    r2 = ftr.reference(Y, PS.astype(np.complex128), 5, 1.5, 0)
    assert r2.bound is None and ftr.check_sets(r2.want.astype(np.complex128) * (1 + 1e-7), r2) < 1.0
    with pytest.raises(ftr.FilterMismatch):
        ftr.check_sets(r2.want.astype(np.complex128) * (1 + 1e-5), r2)


@pytest.mark.parametrize("name", ("single_wu2", "single_unbiased"))
def test_mean_identity_against_golden(golden, name):
    """(1 / M) sum_i x~_i = tsPWS: the mean of the checker's filtered traces against the reference's tsPWS of the 16 x 2048 golden."""
    g = golden["mains"]
    X = _case_input(g, name)
    M, N = X.shape
    assert (M, N) == (16, 2048)
    p = abi.resolve(_case_params(g, name), N, float(g[f"{name}/dt"]))
    assert not p.Kmax and p.wu == 2.0 and bool(p.unbiased) == (name == "single_unbiased")
    fr = irr.Frame.from_oracle(p, N)
    Y = np.stack([fr.oracle.forward(X[i].astype(np.float64)) for i in range(M)])
    PS = ftr.phase_stack(Y)
    x = ftr.filtered_rows(fr, Y, PS, M, p.wu, p.unbiased)
    mean = (x.sum(axis=0) / M).astype(np.float64)
    err = abi.relerr(mean, g[f"{name}/tsPWS"])
    print(name, "relerr of the mean of the filtered traces against tsPWS:", err)
    assert err < ftr.PARITY


def test_group_sums():
    Y = _sets(11, 16, 1)
    G = ftr.group_sums(Y, 4)
    assert np.abs(G.sum(axis=0) - Y.sum(axis=0)).max() < 1e-13
    assert np.abs(G[0] - Y[:3].sum(axis=0)).max() < 1e-13      # floor(i 4 / 11) == 0 for i = 0, 1, 2


def test_filter_plan_check():
    """csrc/filter_plan.h against a direct enumeration, as a stand-alone program under AddressSanitizer + UBSan."""
    pkg = os.path.join(ROOT, "ts-pws_amd")
    exe = os.path.join(pkg, "bin", "filter_plan_check")
    r = subprocess.run(["make", "-C", pkg, "filter_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
