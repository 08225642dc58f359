"""The checker of the trace scores (tspws_hip_trace_scores): per trace the four window sums in np.longdouble from the float32 inputs, and
the bounds a correct FP64 implementation stays inside whatever the order of its sums.  With u = 2**-53 and n the window length:

    |dot - dot*|       <= 1.01 n u sum |x r|        products of two floats are exact in FP64: summation error only
    |xx - xx*|         <= 1.01 n u xx*
    |misfit - misfit*| <= 1.01 (n + 3) u misfit*    the difference and its square are rounded once each, then the summation
    |sim - sim*|       <= (2 n + 8) u  absolute     dot's error over sqrt(xx rr) is at most n u by Cauchy-Schwarz, the two roots carry half
                                                    of xx's and rr's relative error each (n u together), the roots and divisions 4 u more

No tolerance is chosen by hand.  A trace or a reference without energy has sim* = NaN (0 / 0), and the NaN positions must agree."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def window(N, win):
    """(n0, n1) of a window argument: None or (n0, n1), n1 == 0 meaning N."""
    n0, n1 = (0, 0) if win is None else win
    return n0, (n1 or N)


def reference(traces, first, refs, win=None):
    """dict of longdouble arrays for the traces [first[0], first[-1]) of float32 `traces` [mtr][>= N] against float32 `refs` [B][R][>= N]
    (N = refs.shape[-1] unless the window says less): sim, misfit, dot [R][T], energy [T], and the bounds b_sim (a scalar), b_misfit, b_dot
    [R][T], b_energy [T]."""
    first = np.asarray(first, dtype=np.int64)
    B, R = refs.shape[0], refs.shape[1]
    n0, n1 = window(refs.shape[-1], win)
    n = n1 - n0
    T = int(first[-1] - first[0])
    out = {k: np.full((R, T), np.nan, LD) for k in ("sim", "misfit", "dot", "b_misfit", "b_dot")}
    out["energy"], out["b_energy"] = np.full(T, np.nan, LD), np.full(T, np.nan, LD)
    for b in range(B):
        lo, hi = int(first[b]), int(first[b + 1])
        if hi == lo:
            continue
        x = traces[lo:hi, n0:n1].astype(LD)
        c = slice(lo - int(first[0]), hi - int(first[0]))
        xx = (x * x).sum(axis=1)
        out["energy"][c], out["b_energy"][c] = xx, 1.01 * n * U * xx
        for k in range(R):
            r = refs[b, k, n0:n1].astype(LD)
            rr = (r * r).sum()
            dot = (x * r).sum(axis=1)
            mis = ((x - r) ** 2).sum(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["sim"][k, c] = dot / np.sqrt(xx) / np.sqrt(rr)
            out["dot"][k, c], out["misfit"][k, c] = dot, mis
            out["b_dot"][k, c] = 1.01 * n * U * np.abs(x * r).sum(axis=1)
            out["b_misfit"][k, c] = 1.01 * (n + 3) * U * mis
    out["b_sim"] = (2 * n + 8) * U
    return out


def check(scores, energy, want, what=""):
    """Every entry of float64 `scores` [R][3][T] (planes sim, misfit, dot) and `energy` (None or [T]) inside the bounds of `want`
    (reference()); NaN exactly where the checker has NaN.  Prints each worst figure as a fraction of its bound before it asserts."""
    scores = np.asarray(scores)
    sim, mis, dot = scores[:, 0], scores[:, 1], scores[:, 2]
    assert sim.shape == want["sim"].shape, (sim.shape, want["sim"].shape)
    nan = np.isnan(want["sim"].astype(np.float64))
    assert np.array_equal(np.isnan(sim), nan), f"{what}: NaN positions of sim differ"
    assert np.isfinite(mis).all() and np.isfinite(dot).all(), f"{what}: misfit / dot not finite"

    def worst(got, ref, bound):
        err = np.abs(got.astype(LD) - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(err == 0, 0, err / bound)  # (0 of a 0 bound: exact)
        return float(np.max(frac)) if frac.size else 0.0, bool((err <= bound).all())

    figures = {
        "sim": worst(sim[~nan], want["sim"][~nan], want["b_sim"]),
        "misfit": worst(mis, want["misfit"], want["b_misfit"]),
        "dot": worst(dot, want["dot"], want["b_dot"]),
    }
    if energy is not None:
        energy = np.asarray(energy)
        assert np.isfinite(energy).all(), f"{what}: energy not finite"
        figures["energy"] = worst(energy, want["energy"], want["b_energy"])
    print(what, "worst error / bound:", ", ".join(f"{k} {v[0]:.3g}" for k, v in figures.items()))
    for k, (frac, ok) in figures.items():
        assert ok, f"{what}: {k} outside its bound ({frac:.3g} of it)"


def select(score, first, rule, a):
    """numpy restatement of tspws_selection_from_scores: (sel int8 [T], kept uint32 [B])."""
    score = np.asarray(score, dtype=np.float64)
    first = np.asarray(first, dtype=np.int64)
    sel = np.zeros(int(first[-1] - first[0]), np.int8)
    kept = np.zeros(first.size - 1, np.uint32)

    def median(v):
        v = np.sort(v)
        return v[v.size // 2] if v.size % 2 else np.float64(0.5) * (v[v.size // 2 - 1] + v[v.size // 2])

    for b in range(first.size - 1):
        c = slice(int(first[b] - first[0]), int(first[b + 1] - first[0]))
        s = score[c]
        thr = np.float64(a)
        if rule == 1:
            fin = s[np.isfinite(s)]
            if not fin.size:
                continue
            med = median(fin)
            mad = median(np.abs(fin - med))
            with np.errstate(invalid="ignore", over="ignore"):
                thr = med - np.float64(a) * np.float64(1.4826) * mad
        with np.errstate(invalid="ignore"):
            sel[c] = s >= thr
        kept[b] = sel[c].sum()
    return sel, kept


def threshold(score, rule, a):
    """The threshold `select` applies to one ensemble's scores (longdouble in, longdouble arithmetic: the margin test's recomputation)."""
    if rule == 0:
        return LD(a)
    fin = np.sort(score[np.isfinite(score.astype(np.float64))])
    if not fin.size:
        return LD(np.nan)

    def median(v):
        v = np.sort(v)
        return v[v.size // 2] if v.size % 2 else LD(0.5) * (v[v.size // 2 - 1] + v[v.size // 2])

    med = median(fin)
    return med - LD(a) * LD(1.4826) * median(np.abs(fin - med))
