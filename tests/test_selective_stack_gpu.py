"""The selective stack (tspws_hip_selective_stack_batch, Plan.selective_stack_batch) on the GPU, shipped library: synthetic ensembles of
24, 40, 0 and 3 traces of 2048 samples (first[0] = 1) with planted outliers -- a zeroed and a pure-noise trace in the first ensemble, a
negated and a pure-noise trace in the second --, a biased single-stage parameter set and an unbiased one with Kmax = 4 (two-stage for the
large ensembles, single-stage for the ensemble of 3: a mixed batch).  The masks must be those of selection_from_scores on
Plan.trace_scores of the same rows, the rows bit-equal to Plan.subsample_batch with the mask, the counts the mask sums; the zeroed and the
negated trace are rejected under both rules; iters = 1 restacks once, iters = 5 stops early on an unchanged mask; a threshold of -2 keeps
every trace with a finite score, 2 keeps none.  A condition, not a skip: on the longdouble reference scores no trace may lie within the
rounding margin of the threshold the test recomputes (rule 0: (2 n + 8) u, the bound of a score; rule 1: (2 + 2 * 1.4826 |a|) times that,
because median and MAD move with the scores) -- otherwise the comparison of masks would depend on rounding, and the seed has to change."""
import importlib

import numpy as np
import pytest

import abi
import trace_scores_ref as tsr

pytestmark = pytest.mark.gpu

tspws = importlib.import_module("ts-pws_amd")
N = 2048
SIZES = (24, 40, 0, 3)
FIRST = 1 + np.concatenate([[0], np.cumsum(SIZES)])
ZEROED, NOISE0, NEGATED, NOISE1 = 1 + 3, 1 + 17, 1 + 24 + 5, 1 + 24 + 31  # rows of the trace array
PARAMS = {"biased": dict(), "two-stage-unbiased": dict(Kmax=4, unbiased=1)}


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


@pytest.fixture(scope="module")
def traces(lib, torch):
    x = tspws.synth(int(FIRST[-1]) + 1, N, seed=31)
    rng = np.random.default_rng(32)
    x[ZEROED] = 0
    x[NEGATED] = -x[NEGATED]
    for row in (NOISE0, NOISE1):
        x[row] = torch.from_numpy(rng.uniform(-0.5, 0.5, N).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    return x


_plans = {}


def plan_of(kind):
    if kind not in _plans:
        _plans[kind] = tspws.Plan(tspws.resolve(abi.default_params(**PARAMS[kind]), N), N)
    return _plans[kind]


def reference_sim(traces, rows, win=None):
    """The checker's longdouble sim of every trace against row b of `rows` (float32 cuda [B][N])."""
    return tsr.reference(traces.cpu().numpy(), FIRST, rows.cpu().numpy()[:, None, :], win)["sim"][0]


def check_margin(sim, rule, a, n):
    """No finite reference score within the rounding margin of its ensemble's threshold."""
    b = (2 * n + 8) * tsr.U
    margin = b if rule == 0 else (2 + 2 * 1.4826 * abs(a)) * b
    for e in range(len(SIZES)):
        s = sim[int(FIRST[e] - FIRST[0]):int(FIRST[e + 1] - FIRST[0])]
        fin = s[np.isfinite(s.astype(np.float64))]
        if fin.size:
            gap = np.abs(fin - tsr.threshold(s, rule, a)).min()
            print(f"ensemble {e}: smallest distance to the threshold {float(gap):.3g}, margin {margin:.3g}")
            assert gap > margin, "a score within rounding of the threshold: change the seed"


def check_pass(torch, plan, traces, rows, against, rule, a, sel, win=None):
    """`sel` is the mask that selection_from_scores gives for Plan.trace_scores against `rows`; returns the sim plane (numpy)."""
    sc = plan.trace_scores(traces, FIRST, rows[0 if against == "ls" else 1], window=win)
    sim = sc[0, 0].cpu().numpy()
    want_sel, want_kept = tspws.selection_from_scores(sim, FIRST, rule, a)
    r = tspws.RULES[rule]
    assert np.array_equal(want_sel, tsr.select(sim, FIRST, r, a)[0])
    n0, n1 = tsr.window(N, win)
    check_margin(reference_sim(traces, rows[0 if against == "ls" else 1], win), r, a, n1 - n0)
    assert np.array_equal(sel, want_sel), (sel.tolist(), want_sel.tolist())
    return sim, want_kept


def threshold_for(sim):
    """Rule 0's threshold of a run: three quarters of the smallest ensemble median of the plain-stack scores."""
    meds = [np.nanmedian(sim[int(FIRST[e] - FIRST[0]):int(FIRST[e + 1] - FIRST[0])]) for e in range(len(SIZES)) if SIZES[e]]
    return 0.75 * float(min(meds))


@pytest.mark.parametrize("rule", ["mad", "threshold"])
@pytest.mark.parametrize("against", ["ts", "ls"])
@pytest.mark.parametrize("kind", list(PARAMS))
def test_selective_stack(lib, torch, traces, kind, against, rule):
    plan = plan_of(kind)
    rows0 = plan.stack_batch(traces, FIRST)
    torch.cuda.synchronize()
    sim0 = plan.trace_scores(traces, FIRST, rows0[0 if against == "ls" else 1])[0, 0].cpu().numpy()
    a = 3.0 if rule == "mad" else threshold_for(sim0)
    print(f"{kind}, against {against}, rule {rule}, a = {a:.4g}; plain-stack sims of the planted rows: zeroed {sim0[ZEROED - 1]:.3g}, negated "
          f"{sim0[NEGATED - 1]:.3g}, noise {sim0[NOISE0 - 1]:.3g} {sim0[NOISE1 - 1]:.3g}; ensemble medians "
          f"{[round(float(np.nanmedian(sim0[int(FIRST[e] - 1):int(FIRST[e + 1] - 1)])), 3) for e in range(4) if SIZES[e]]}")

    # one pass
    ls, ts, sel, kept, done = plan.selective_stack_batch(traces, FIRST, against=against, rule=rule, a=a, iters=1)
    assert done == 1 and sel.shape == (int(FIRST[-1] - FIRST[0]),) and set(np.unique(sel)) <= {0, 1}
    _, want_kept = check_pass(torch, plan, traces, rows0, against, rule, a, sel)
    assert sel[ZEROED - 1] == 0 and sel[NEGATED - 1] == 0  # the dead and the negated trace are rejected
    sums = np.array([sel[int(FIRST[e] - 1):int(FIRST[e + 1] - 1)].sum() for e in range(4)], np.uint32)
    assert np.array_equal(kept, sums) and np.array_equal(kept, want_kept) and kept[2] == 0
    ls_m, ts_m, mtr_m = plan.subsample_batch(traces, FIRST, sel[None])
    assert torch.equal(ls, ls_m[:, 0]) and torch.equal(ts, ts_m[:, 0]) and np.array_equal(mtr_m[:, 0], kept)
    assert not bool(ls[2].any()) and not bool(ts[2].any())  # the empty ensemble: zero rows

    # up to five restacks: stops early, and the mask it stopped on is what its final rows select again
    ls5, ts5, sel5, kept5, done5 = plan.selective_stack_batch(traces, FIRST, against=against, rule=rule, a=a, iters=5)
    print(f"iters = 5: {done5} restacks, kept {kept5.tolist()} (one pass: {kept.tolist()})")
    assert 1 <= done5 < 5
    check_pass(torch, plan, traces, (ls5, ts5), against, rule, a, sel5)
    ls_m, ts_m, mtr_m = plan.subsample_batch(traces, FIRST, sel5[None])
    assert torch.equal(ls5, ls_m[:, 0]) and torch.equal(ts5, ts_m[:, 0]) and np.array_equal(mtr_m[:, 0], kept5)
    assert sel5[ZEROED - 1] == 0 and sel5[NEGATED - 1] == 0
    if done5 == 1:
        assert np.array_equal(sel5, sel)


@pytest.mark.parametrize("kind", list(PARAMS))
def test_threshold_extremes_and_window(lib, torch, traces, kind):
    plan = plan_of(kind)
    rows0 = plan.stack_batch(traces, FIRST)
    sim0 = plan.trace_scores(traces, FIRST, rows0[1])[0, 0].cpu().numpy()
    # -2 is below every similarity: every trace with a finite score is kept (the zeroed one has none)
    ls, ts, sel, kept, done = plan.selective_stack_batch(traces, FIRST, rule="threshold", a=-2.0, iters=3)
    assert np.array_equal(sel.astype(bool), np.isfinite(sim0)) and sel.sum() == sum(SIZES) - 1 and sel[ZEROED - 1] == 0
    assert kept.tolist() == [SIZES[0] - 1, SIZES[1], 0, SIZES[3]] and 1 <= done <= 3
    # 2 is above every similarity: nothing is kept, zero rows, zero counts; the second pass scores against zero rows (NaN) and selects nothing again
    ls, ts, sel, kept, done = plan.selective_stack_batch(traces, FIRST, rule="threshold", a=2.0, iters=3)
    assert not sel.any() and not kept.any() and done == 1
    assert not bool(ls.any()) and not bool(ts.any())
    # a lag window: the masks follow the scores of that window
    win = (N // 2 - 300, N // 2 + 301)
    ls, ts, sel, kept, done = plan.selective_stack_batch(traces, FIRST, against="ls", rule="mad", a=3.0, iters=1, window=win)
    check_pass(torch, plan, traces, rows0, "ls", "mad", 3.0, sel, win)
    assert done == 1 and sel[ZEROED - 1] == 0
    # refusals with a plan: outputs of the binding aside, the C call returns -1 with its own text
    for kw in (dict(against="both"), dict(rule="median")):
        with pytest.raises(tspws.TspwsError):
            plan.selective_stack_batch(traces, FIRST, **kw)
    with pytest.raises(tspws.TspwsError, match="selective_stack_batch"):
        plan.selective_stack_batch(traces, FIRST, iters=0)
    with pytest.raises(tspws.TspwsError, match="lag window"):
        plan.selective_stack_batch(traces, FIRST, window=(0, N + 1))
