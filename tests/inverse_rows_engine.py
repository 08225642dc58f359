"""Cases and runner of tests/test_inverse_rows_gpu.py, and its child process: `python inverse_rows_engine.py GROUP` runs the sweeps-build cases
of one group in a FRESH process, because TSPWS_INV_SPLIT, TSPWS_INV_LDS, TSPWS_INV_LDS_MAXD and TSPWS_INV_GENERIC are read once per process
by the library (the parent sets them, and TSPWS_LIB_PATH).  The case list and the coefficient sets need no GPU (tests/test_inverse_rows_cpu.py
holds the cap of every case); everything that runs a case does (marked gpu through test_inverse_rows_gpu.py).

A case = one frame and one list of coefficient sets, all through ONE tspws_hip_inverse call (Plan.inverse) and held to the CPU reference at
every sample of every row (inverse_rows_ref.check_rows):

    F full sets        white complex-normal coefficients, each with one stretch of exact zeros and one subnormal
    S single-scale sets set s carries scale s of full set 0 only: its row is that scale's share of row 0, checked on its own
    impulse sets       one coefficient (one non-zero component) at k = 0, N_s - 1 or N_s / 2 of the first scale of every octave, of every scale
                       where the kernel body changes, and of the coarsest scale

then the first 1, 2, 3, 4 and 7 sets in calls of their own (NREC = 1 alone, one pair, pair + single, two pairs -- where the LDS-staged form
switches on --, three pairs + single), the first 7 sets one by one (is set r of a larger call bit-identical to the same set alone?) and
the properties that need no tolerance.  Before any call the case asserts its route: tspws_hip_inverse_info must answer what
inverse_rows_ref.launch_list derives from the tables by the documented rule, and the frame must have the forms the case is there for.

Every case prints one line `INVERSE_ROWS group: case | route | cap ratio | worst ratio ... | bit-identity ...` and appends it to the file named
by TSPWS_INVERSE_REPORT when that is set.  The child also prints `INVERSE_ROWS_DIGEST group case sha256` (of all its result rows) and ends
with `INVERSE_ROWS_DONE group passed failed`; a case that fails its bound is reported and the child goes on (a numerical miss is no device
fault), any other error ends it."""
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
import abi
from inverse_rows_ref import Frame, assemble, check_rows, launch_list, reference_rows

COUNTS = (1, 2, 3, 4, 7)
BIG_SETS = 65539          # 32768 pairs (one full chunk of grid.y) + one pair + the odd set


def case(kw, N, seed, expect, F=3):
    return dict(kw=kw, N=N, seed=seed, expect=expect, F=F)


def name_of(c):
    kw = ",".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in c["kw"].items()) or "default"
    return f"N = {c['N']} [{kw}] F = {c['F']}"


# expect: per_scale; gen = "none" / "all D > 1"; lds = "none" / "D = 1"; D = the decimations; chunks = 64-phase chunks of the wave-uniform
# scales; idle: some wave-uniform scale with D % 64 != 0; lds_blocks = (most blocks of 32 tap steps, a partial last block somewhere);
# lds_short: N_s shorter than the staged window (the row %= Ns branch); Lmax
CASES = [
    case(dict(), 4096, 11, dict(per_scale=1, gen="none", lds="none", D=[2, 4, 8, 16, 32, 64, 128, 256, 512], chunks=[1, 2, 4, 8])),
    case(dict(), 4097, 12, dict(per_scale=1, gen="all D > 1", lds="none", D=[2, 4, 8, 16, 32, 64, 128, 256, 512], partial_last_row=True)),
    case(dict(s0=3.7, J=5), 3001, 13, dict(per_scale=1, gen="all D > 1", lds="none", D=[3, 7, 14, 29, 59], partial_last_row=True)),
    case(dict(b0=3.0), 3072, 14, dict(per_scale=1, gen="none", lds="none", D=[6, 12, 24, 48, 96, 192, 384, 768], chunks=[2, 3, 6, 12], idle=True)),
    case(dict(type=-3), 2048, 15, dict(per_scale=1, gen="none", lds="D = 1", D=[1, 2, 4, 8, 16, 32], lds_blocks=(1, True))),
    case(dict(b0=0.25), 4096, 16, dict(per_scale=1, gen="none", lds="D = 1", D=[1, 2, 4, 8, 16, 32, 64, 128], chunks=[1, 2], lds_blocks=(3, True), qmin=40, qmax=69)),
    case(dict(uni=1, J=4), 1024, 17, dict(per_scale=1, gen="none", lds="D = 1", D=[1], lds_blocks=(9, True), Lmax=271)),
    case(dict(type=-3, J=2), 256, 18, dict(per_scale=1, gen="none", lds="D = 1", D=[1], lds_short=True)),
    case(dict(uni=1, J=3), 256, 19, dict(per_scale=1, gen="none", lds="D = 1", D=[1], lds_short=True, lds_blocks=(5, True))),
    case(dict(), 32768, 20, dict(per_scale=0, gen="none", lds="none", waves=768, items=12, chunks=[1, 2, 4, 8, 16, 32, 64]), F=2),
    case(dict(J=2), 64, 21, dict(per_scale=1, gen="none", lds="none", D=[2, 4])),
]
BIG = CASES[-1]

# ---- sweeps build: name -> (environment, keywords of launch_list, what the switch must have done)
SWEEP_CASES = [CASES[0], CASES[4], CASES[1]]
GROUPS = {
    "default": (dict(), dict(), dict()),
    "split0": (dict(TSPWS_INV_SPLIT="0"), dict(split=False), dict(per_scale=0)),
    "split1": (dict(TSPWS_INV_SPLIT="1"), dict(split=True), dict(per_scale=1)),
    "lds0": (dict(TSPWS_INV_LDS="0"), dict(lds=False), dict(waves_lds=0)),
    "maxd32": (dict(TSPWS_INV_LDS_MAXD="32"), dict(lds_maxd=32), dict(lds_all_up_to=32)),
    "generic": (dict(TSPWS_INV_GENERIC="1"), dict(generic=True), dict(generic=1)),
}
SWITCHES = ("TSPWS_INV_SPLIT", "TSPWS_INV_LDS", "TSPWS_INV_LDS_MAXD", "TSPWS_INV_GENERIC")
CHILD_TIMEOUT = 600


# ------------------------------------------------------------------------------------------------------------------------------------ data --
def classes_of(fr, route):
    """Per scale: what distinguishes the code a scale runs through -- body, decimation, blocks of 32 staged tap steps."""
    return [(route["body"][s], int(fr.D[s]), -(-(-(-int(fr.L[s]) // int(fr.D[s]))) // 32) if route["body"][s] == "LDS-staged" else 0) for s in range(fr.S)]


def impulse_scales(fr):
    cl = classes_of(fr, launch_list(fr))
    return sorted({0, fr.S - 1} | {s for s in range(1, fr.S) if cl[s] != cl[s - 1]})


def sets_of(c, fr):
    """The case's coefficient sets (see the module docstring), seeded: F full, S single-scale, the impulses -- in that order."""
    rng = np.random.default_rng(c["seed"])
    S, off, Ns = fr.S, fr.off, fr.Ns
    sets = []
    for i in range(c["F"]):
        Y = rng.standard_normal(fr.ncoef) + 1j * rng.standard_normal(fr.ncoef)
        sz = (S // 2 + i) % S                       # a stretch of exact zeros inside one scale (never the whole scale)
        a = int(off[sz]) + int(Ns[sz]) // 3
        Y[a: a + max(1, int(Ns[sz]) // 4)] = 0
        Y[int(off[i % S]) + 1] = complex(1e-310, 0)  # a subnormal
        sets.append(("full", Y))
    for s in range(S):
        sets.append(("scale", s, sets[0][1][off[s]: off[s + 1]].copy()))
    values = (complex(1.5, 0), complex(0, -0.75), complex(-1.25, 0))
    for s in impulse_scales(fr):
        for j, k in enumerate(sorted({0, int(Ns[s]) - 1, int(Ns[s]) // 2})):
            sets.append(("impulse", s, k, values[j % 3]))
    return sets


_refs = {}


def reference_of(c, fr, key_extra=""):
    """(sets, Y[R][ncoef], reference) of a case for the frame `fr` (its taps are part of the key: the device's or the oracle's)."""
    key = (tuple(sorted(c["kw"].items())), c["N"], c["seed"], c["F"], key_extra)
    if key not in _refs:
        sets = sets_of(c, fr)
        _refs[key] = (sets, assemble(fr, sets), reference_rows(fr, sets))
    return _refs[key]


# ----------------------------------------------------------------------------------------------------------------------------------- route --
def route_text(r, fr):
    gen = sum(1 for b in r["body"] if b == "GEN")
    lds = sum(1 for b in r["body"] if b == "LDS-staged")
    uni = sorted({r["chunks"][s] for s in range(fr.S) if r["body"][s] == "wave-uniform"})
    what = "k_inverse_generic" if r["generic"] else (f"{r['items']} items {'per scale' if r['per_scale'] else 'per octave'}, {r['waves']} waves: "
                                                    f"LDS-staged {r['waves_lds']} ({lds} scales), GEN {r['waves'] - r['waves_fast']} ({gen} scales)"
                                                    + (f", wave-uniform chunks {uni}" if uni else ""))
    return f"D {int(fr.D.min())}..{int(fr.D.max())} L {int(fr.L.min())}..{int(fr.L.max())} | {what}"


def assert_route(c, info, r, fr, must=None):
    """info = tspws_hip_inverse_info's answer, r = launch_list's; c['expect'] (shipped rule) or `must` (a sweeps switch) = the forms the case is there for."""
    what = (name_of(c), info, {k: v for k, v in r.items() if k not in ("body", "chunks")})
    for k in ("items", "per_scale", "waves", "waves_lds", "waves_fast", "generic"):
        assert info[k] == r[k], (k,) + what
    D, L, Ns, N = fr.D, fr.L, fr.Ns, fr.N
    Q = -(-L // D)
    gen = [s for s in range(fr.S) if N % int(D[s])]
    d1 = [s for s in range(fr.S) if int(D[s]) == 1]
    if must is not None:
        for k in ("per_scale", "waves_lds", "generic"):
            if k in must:
                assert info[k] == must[k], (k,) + what
        if "lds_all_up_to" in must:     # every scale whose D divides N and is <= 32 is staged (they come first in the list), no other
            staged = [s for s in range(fr.S) if r["body"][s] == "LDS-staged"]
            assert staged == [s for s in range(fr.S) if N % int(D[s]) == 0 and int(D[s]) <= must["lds_all_up_to"]], what
            assert (info["waves_lds"] > 0) == bool(staged), what
        return
    e = c["expect"]
    assert info["generic"] == 0 and info["per_scale"] == e["per_scale"], what
    if e["gen"] == "none":
        assert not gen and info["waves_fast"] == info["waves"], what
    else:
        assert gen and gen == [s for s in range(fr.S) if int(D[s]) > 1] and all(r["body"][s] == "GEN" for s in gen), what
        assert info["waves"] > info["waves_fast"] and (len(gen) < fr.S or info["waves_fast"] == 0), what
    if e["lds"] == "none":
        assert not d1 and info["waves_lds"] == 0, what
    else:           # the D = 1 scales: 64 groups of 8 outputs per wave
        assert d1 and info["waves_lds"] == sum(-(-int(Ns[s]) // 512) for s in d1) and all(r["body"][s] == "LDS-staged" for s in d1), what
    if "D" in e:
        assert sorted(set(D.tolist())) == e["D"], what
    uni = [s for s in range(fr.S) if r["body"][s] == "wave-uniform"]
    if "chunks" in e:
        assert uni == [s for s in range(fr.S) if int(D[s]) >= 64 and N % int(D[s]) == 0] and sorted({r["chunks"][s] for s in uni}) == e["chunks"], what
    if e.get("idle"):
        assert any(int(D[s]) % 64 for s in uni) and any(int(D[s]) & (int(D[s]) - 1) for s in range(fr.S)), what
    if e.get("partial_last_row"):
        assert all(int(Ns[s]) * int(D[s]) > N for s in gen), what
    if "lds_blocks" in e:
        assert max(-(-int(Q[s]) // 32) for s in d1) == e["lds_blocks"][0] and any(int(Q[s]) % 32 for s in d1) == e["lds_blocks"][1], what
    if e.get("lds_short"):       # rows the first staged block can touch: 64 groups x 8 + 2 + its steps rounded up to 8 + 8
        assert all(int(Ns[s]) < 64 * 8 + 2 + -(-min(int(Q[s]), 32) // 8) * 8 + 8 for s in d1), what
    if "qmin" in e:
        assert min(int(Q[s]) for s in range(fr.S) if 1 < int(D[s]) < 64) >= e["qmin"] and int(Q.max()) == e["qmax"], what
    if "Lmax" in e:
        assert int(L.max()) == e["Lmax"], what
    for k in ("waves", "items"):
        if k in e:
            assert info[k] == e[k], what


# ------------------------------------------------------------------------------------------------------------------------------------- run --
def report(line):
    print(line, flush=True)
    path = os.environ.get("TSPWS_INVERSE_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def sweep_keywords(tp):
    """launch_list's keywords from the switches the loaded library reads (the sweeps build only; the shipped one ignores them)."""
    if not tp.LIB_PATH.endswith("_sweeps.so"):
        return {}
    kw, env = {}, os.environ
    if env.get("TSPWS_INV_SPLIT") is not None:
        kw["split"] = int(env["TSPWS_INV_SPLIT"]) != 0
    if env.get("TSPWS_INV_LDS", "")[:1] == "0":
        kw["lds"] = False
    if env.get("TSPWS_INV_LDS_MAXD") is not None:
        kw["lds_maxd"] = max(0, int(env["TSPWS_INV_LDS_MAXD"]))
    if env.get("TSPWS_INV_GENERIC", "")[:1] == "1":
        kw["generic"] = True
    return kw


def run_case(tp, c, group="shipped", must=None):
    """One case on the module `tp` (the binding over the shipped or the sweeps library).  Raises on a wrong route or a sample outside its bound;
    returns dict(worst, cap, differs, digest)."""
    N = c["N"]
    pl = tp.Plan(tp.resolve(abi.default_params(**c["kw"]), N), N)
    fr = Frame.from_plan(pl)
    route = launch_list(fr, **sweep_keywords(tp))
    info = pl.inverse_info()
    assert_route(c, info, route, fr, must)
    sets, Y, ref = reference_of(c, fr, key_extra=hashlib.sha256(fr.wd.tobytes()).hexdigest())
    text = route_text(route, fr)
    R = len(sets)
    assert R >= max(COUNTS) and ref.cap_ratio < 1e-12
    sha = hashlib.sha256()
    worst, by_kind = dict(ratio=-1.0), {}

    def held(x, rows, nsets, what):
        sha.update(x.tobytes())
        try:
            w = check_rows(x, ref, rows=rows, route=route, nsets=nsets)
        except AssertionError as err:
            report(f"INVERSE_ROWS_FAIL {group}: {name_of(c)} | {text} | {what}: {err}")
            raise
        for k, v in w["by_kind"].items():
            by_kind[k] = max(by_kind.get(k, 0.0), v)
        if w["ratio"] > worst["ratio"]:
            worst.update(w, what=what, row=rows[w["row"]])

    x_all = pl.inverse(Y)
    held(x_all, list(range(R)), R, f"all {R} sets")
    calls = {R: x_all}
    for n in COUNTS:
        calls[n] = pl.inverse(Y[:n])
        held(calls[n], list(range(n)), n, f"first {n} set(s)")
    solo = [pl.inverse(Y[r: r + 1]) for r in range(max(COUNTS))]
    for r, x in enumerate(solo):
        held(x, [r], 1, f"set {r} alone")
    # is set r of a larger call bit-identical to the same set in a call of its own?  (reported; a difference inside the bound is no failure)
    differs = [(n, r) for n in sorted(calls) for r in range(min(n, max(COUNTS))) if calls[n][r].tobytes() != solo[r][0].tobytes()]
    # no tolerance: the same call twice; an all-zero set gives a zero row; a set scaled by 2 gives exactly twice the row (two pairs: the
    # LDS-staged form where the frame has one; and the odd single set)
    for n in (max(COUNTS), R):
        assert pl.inverse(Y[:n]).tobytes() == calls[n].tobytes(), (name_of(c), text, f"the same call of {n} sets twice")
    Yx = np.stack([Y[0], np.zeros_like(Y[0]), Y[1], 2 * Y[0], 2 * Y[2 % c["F"]]])
    xx = pl.inverse(Yx)
    assert not np.isnan(xx).any() and not xx[1].any(), (name_of(c), text, "an all-zero set gives a zero row")
    assert xx[3].tobytes() == (2 * xx[0]).tobytes(), (name_of(c), text, "a set scaled by 2 (in a pair)")
    assert xx[4].tobytes() == (2 * solo[2 % c["F"]][0]).tobytes(), (name_of(c), text, "a set scaled by 2 (the odd last set)")
    assert worst["ratio"] <= 1
    where = f"row {worst['row']}" + (f" scale {worst['scale']}" if worst["scale"] is not None else " (full set)") + f" sample {worst['sample']}, {worst['what']}"
    ident = "every set of a larger call bit-identical to the set alone" if not differs else \
        f"NOT bit-identical to the set alone: (sets in call, set) {differs[:12]}{' ...' if len(differs) > 12 else ''}"
    report(f"INVERSE_ROWS {group}: {name_of(c)} | {text} | {R} sets | cap ratio {ref.cap_ratio:.2e} | worst |diff| / bound {worst['ratio']:.3g} @ {where} "
           f"(full sets {by_kind['full']:.3g}, single-scale {by_kind['scale']:.3g}, impulses {by_kind['impulse']:.3g}) | {ident}; "
           f"twice / zero set / x2 exact")
    return dict(worst=worst, by_kind=by_kind, cap=ref.cap_ratio, differs=differs, digest=sha.hexdigest())


def run_big(tp, group="shipped"):
    """More than 32768 pairs in one call: BIG_SETS sets built on the device as cyclic copies of the first 8 sets of the smallest case.  Rows
    0 .. 7 go through the checker; every other row must be bit-identical to its template row."""
    import torch
    c, N = BIG, BIG["N"]
    pl = tp.Plan(tp.resolve(abi.default_params(**c["kw"]), N), N)
    fr = Frame.from_plan(pl)
    route = launch_list(fr, **sweep_keywords(tp))
    assert_route(c, pl.inverse_info(), route, fr)
    sets, Y, ref = reference_of(c, fr, key_extra=hashlib.sha256(fr.wd.tobytes()).hexdigest())
    T = 8
    Yd = torch.as_tensor(Y[:T], device="cuda").repeat(-(-BIG_SETS // T), 1)[:BIG_SETS].contiguous()
    assert tuple(Yd.shape) == (BIG_SETS, pl.ncoef) and BIG_SETS // 2 > 32768 and BIG_SETS % 2
    x = pl.inverse(Yd)
    w = check_rows(x[:T].cpu().numpy(), ref, rows=list(range(T)), route=route, nsets=BIG_SETS)
    bits = x.view(torch.int64)
    same = (bits == bits[:T].repeat(-(-BIG_SETS // T), 1)[:BIG_SETS]).all(dim=1)
    bad = torch.nonzero(~same).flatten().cpu().numpy().tolist()
    border = list(range(BIG_SETS - 5, BIG_SETS))        # the last pair of the full chunk, the pair behind it, the odd tail
    assert not bad, (f"{len(bad)} of {BIG_SETS} rows differ from their template row (row mod {T}); first {bad[:8]}; of the chunk border and odd tail "
                     f"{border}: {[r for r in border if r in set(bad)]}")
    report(f"INVERSE_ROWS {group}: {BIG_SETS} sets of {name_of(c)} (cyclic copies of 8) | {route_text(route, fr)} | cap ratio {ref.cap_ratio:.2e} | "
           f"worst |diff| / bound {w['ratio']:.3g} @ row {w['row']} sample {w['sample']} of rows 0..7 | rows 8..{BIG_SETS - 1} bit-identical to their templates "
           f"(chunk border and odd tail {border[0]}..{border[-1]} included)")
    return w


def main(group):
    env, _, must = GROUPS[group]
    for k in SWITCHES:
        assert os.environ.get(k) == env.get(k), f"the parent sets {k} to {env.get(k)}"
    tp = importlib.import_module("ts-pws_amd")
    assert tp.LIB_PATH.endswith("_sweeps.so"), tp.LIB_PATH
    assert tp.load().tspws_hip_device_count() > 0
    ok = bad = 0
    for c in SWEEP_CASES:
        try:
            r = run_case(tp, c, group, must)
            print(f"INVERSE_ROWS_DIGEST {group} {name_of(c).replace(' ', '')} {r['digest']}", flush=True)
            ok += 1
        except AssertionError as err:
            bad += 1
            print(f"INVERSE_ROWS_ASSERT {group}: {name_of(c)}: {err}", flush=True)
    print(f"INVERSE_ROWS_DONE {group} {ok} {bad}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
