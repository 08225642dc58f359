"""Cases and runner of tests/test_stack_planes_gpu.py, and its child process: `python stack_planes_engine.py GROUP` runs the cases of one
group in a FRESH process, because TSPWS_ENGINE, TSPWS_PART_MB, TSPWS_GEMM_ORDER and TSPWS_SPEC_NSMAX are read once per process by the library
(the parent sets them, and TSPWS_LIB_PATH for the groups that need the sweeps build).

A case = one call of Plan.stacks (tspws_hip_stacks_float / tspws_hip_stacks_double) on seeded rows, held to the CPU reference planes at
every coefficient (stack_planes_ref.check_planes).  Before the call the case asserts the route it is meant to take, from the library's own
answers (tspws_hip_spectral_choice, tspws_hip_spectral_end_scale, tspws_hip_spectral_transform_length, the frame tables) and the documented
size rule of the trace-lane path, so that a change of the selection rule cannot silently empty it.

Every case prints one line `STACK_PLANES case route max_bPS rST@scale rPS@scale` and appends it to the file named by TSPWS_PLANES_REPORT when
that is set.  The child ends with `STACK_PLANES_DONE group passed failed`; a case that fails its bound is reported and the child goes on (a
numerical miss is no device fault), any other error ends it."""
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
from stack_planes_ref import check_planes, punch_holes, reference_planes

TWO_PI = 2 * np.pi


def case(kw, M, N, seed, expect, holes=False, f64=False, rows=None, tag="", carrier=None):
    """rows = K: the K FP64 partial stacks (orc_partial_stacks) of 900 seeded traces instead of M traces (then M = K, f64).
    carrier: amplitude of a Nyquist carrier a * (-1)^n added to every trace -- the data of the w0 = 2 pi frames (default there: 2).  Their
    finest scale (s0 = 2) sits AT the Nyquist frequency, where the filter's imaginary part vanishes: the coefficients of noise are real,
    |Y| is the modulus of ONE Gaussian variable instead of two and comes arbitrarily close to 0 with a probability linear in the distance, so on
    abi.synth_traces alone the phasors of that scale are ill conditioned (max bPS 2e-6 .. 1e-4 over seeds: outside the 1e-6 cap of
    stack_planes_ref.py).  The carrier (4 times the noise's amplitude) keeps every coefficient of the finest scales away from 0."""
    if carrier is None:
        carrier = 2.0 if kw.get("w0") == TWO_PI else 0.0
    return dict(kw=kw, M=rows or M, N=N, seed=seed, expect=expect, holes=holes, f64=f64 or bool(rows), rows=rows, tag=tag, carrier=carrier)


def exact(kw, M, N, seed, f64=False):
    return dict(kw=kw, M=M, N=N, seed=seed, exact=True, f64=f64, carrier=0.0)


def name_of(c):
    kw = ",".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in c["kw"].items()) or "default"
    what = "exact " if c.get("exact") else ""
    src = f"{c['rows']} f64 partial rows" if c.get("rows") else f"{c['M']}" + (" f64" if c["f64"] else "")
    return f"{what}{src} x {c['N']} [{kw}]" + (" holes" if c.get("holes") else "") + (" +carrier" if c.get("carrier") else "") + (f" {c['tag']}" if c.get("tag") else "")


SPEC = dict(path="spectral")
FEW = dict(path="few")

# ---- shipped library, default rule (in process): D >= 32 octaves spectral (two-voice frames: D >= 16), finer ones on k_fwd_tl, clipped scales
# on the contraction
DEFAULT = [
    case(dict(), 499, 16501, 21, dict(path="spectral", dmin=32, gemm=5, NT=32768, last=51)),      # the reference's own data shape
    case(dict(), 300, 4097, 22, dict(path="spectral", dmin=32, gemm=5, NT=8192, pow2=False), holes=True),   # window nearly twice the trace
    case(dict(), 300, 4096, 23, dict(path="spectral", dmin=32, gemm=0, NT=4096)),
    case(dict(), 257, 8192, 24, dict(path="spectral", dmin=32, gemm=0, last=1)),                    # five blocks, the last with one trace
    case(dict(), 257, 8192, 24, dict(path="spectral", dmin=32, gemm=0, last=1), f64=True),          # the same rows as float64 input
    case(dict(), 64, 16384, 25, dict(path="spectral", dmin=32, gemm=0, last=64)),                   # one block at the 1 M-sample threshold
    case(dict(w0=TWO_PI), 260, 1501, 26, dict(path="spectral", dmin=32, pow2=False)),               # odd N: no decimation divides it
    case(dict(type=-3), 256, 3000, 27, dict(path="spectral", dmin=16, pow2=False)),                 # Mexican hat: the D >= 16 set
    case(dict(type=-3), 70, 20000, 28, dict(path="spectral", dmin=16, pow2=False)),
    case(dict(type=-2), 300, 5000, 29, dict(path="spectral", dmin=32, gemm=6, NT=8192, pow2=False)),
    case(dict(b0=4.0), 66, 16384, 30, dict(path="spectral", dmin=32, gemm=0)),
    case(dict(V=7), 300, 4096, 31, dict(path="spectral", dmin=32, gemm=0, V=7)),
]

# ---- few-trace fused form of k_fwd_lds (shipped library): slice counts on both sides of every fuse_tps step
FEW_FUSED = [case(dict(), M, N, 40 + M, FEW) for N in (2048, 8192, 16501) for M in (1, 2, 3, 7, 31, 32, 33, 63)]

# ---- float64 rows (tspws_hip_stacks_double): the K partial stacks of a two-stage call
DOUBLE_DEFAULT = [
    case(dict(), 0, 4097, 51, dict(path="spectral", dmin=32, pow2=False), rows=300),    # from 256 rows on the default rule takes the spectral route
    case(dict(), 0, 16501, 52, FEW, rows=10),                                          # the headline's finish stage: ONE fused slice straight into ST / PS
    case(dict(), 0, 131072, 53, FEW, rows=10),
]
DOUBLE_SMALL = [(K, N) for K in (80, 200) for N in (2048, 4097)]

EXACT_DEFAULT = [exact(dict(), 7, 8192, 61), exact(dict(), 33, 2048, 62), exact(dict(), 300, 4097, 63), exact(dict(), 64, 16384, 64),
                 exact(dict(type=-3), 256, 3000, 65), exact(dict(), 300, 4096, 66, f64=True)]

# ---- groups that run in a child process: name -> (environment, sweeps build?, timeout of the child in s, cases)
GROUPS = {
    "spectral": (dict(TSPWS_ENGINE="spectral"), False, 900, [
        case(dict(), 66, 16501, 71, dict(path="spectral", gemm=5, NT=32768)),
        case(dict(), 100, 3000, 72, SPEC, holes=True),
        case(dict(w0=TWO_PI), 130, 1501, 73, SPEC),
        case(dict(), 64, 1024, 74, SPEC),
        case(dict(V=7, J=6), 90, 4096, 75, dict(path="spectral", V=7)),
    ] + [case(dict(), 0, N, 76, SPEC, rows=K) for K, N in DOUBLE_SMALL] + [exact(dict(), 100, 3000, 77)]),
    "fir": (dict(TSPWS_ENGINE="fir"), False, 1200, [
        case(dict(), 256, 32768, 81, dict(path="tl", pick=1, blocks=4)),
        case(dict(), 800, 16384, 5, dict(path="tl", pick=0, blocks=13, last=32)),
        case(dict(), 450, 16501, 83, dict(path="tl", pick=1)),       # 7.4 M samples, just over the 7 x 2^20 rule; clipped scales on k_fwd_poly<.,2>
        exact(dict(), 450, 16501, 84),
    ]),
    # TSPWS_PART_MB=16 (the smallest the library accepts): a trace's partials take >= ncoef * 16 bytes, so stacks_impl walks >= 4 batches with a
    # shorter last one and adds the planes under `keep`.  By the default rule 100 x 16501 (>= 64 traces, >= 1 M samples) is a many-trace batch, so
    # the few-trace batches of M = 100 need the FIR pin as well; without it 100 / 300 x 16501 size the batches of the trace-lane pass.
    "partmb_fir": (dict(TSPWS_PART_MB="16", TSPWS_ENGINE="fir"), False, 900, [
        case(dict(), 63, 16501, 91, dict(path="few", batches=4)),
        case(dict(), 100, 16501, 92, dict(path="few", batches=4)),
        case(dict(), 40, 65536, 93, dict(path="few", batches=4)),
        exact(dict(), 63, 16501, 94),
    ]),
    "partmb": (dict(TSPWS_PART_MB="16"), False, 900, [
        case(dict(), 63, 16501, 91, dict(path="few", batches=4)),
        case(dict(), 40, 65536, 93, dict(path="few", batches=4)),
        case(dict(), 100, 16501, 92, dict(path="spectral", gemm=5)),
        case(dict(), 300, 16501, 95, dict(path="spectral", gemm=5)),
    ]),
    "nsmax": (dict(TSPWS_SPEC_NSMAX=str(1 << 30)), True, 600, [          # every octave with D >= 8 spectral
        case(dict(), 300, 4096, 23, dict(path="spectral", dfirst=8, gemm=0)),
        case(dict(), 257, 8192, 24, dict(path="spectral", dfirst=8, gemm=0)),
    ]),
}
for _o in (0, 1, 2):   # the contraction in front of / behind / beside the trace-lane kernel
    GROUPS[f"gemm{_o}"] = (dict(TSPWS_GEMM_ORDER=str(_o)), True, 600, [case(dict(), 300, 4097, 22, dict(path="spectral", pow2=False), holes=True, tag=f"TSPWS_GEMM_ORDER={_o}")])


# ------------------------------------------------------------------------------------------------------------------------------------ data --
def partial_rows(K, N, seed, total=900):
    """The K FP64 partial stacks (oracle: orc_partial_stacks) of `total` seeded traces, generated 100 at a time."""
    X = np.empty((total, N), np.float32)
    for t0 in range(0, total, 100):
        X[t0: t0 + 100] = abi.synth_traces(min(100, total - t0), N, seed=seed, first=t0)
    P = np.zeros((K, N), np.float64)
    abi.oracle().orc_partial_stacks(P.ctypes.data, X.ctypes.data, N, total, K)
    return P


def rows_of(c):
    if c.get("rows"):
        X = partial_rows(c["rows"], c["N"], c["seed"])
    else:
        X = abi.synth_traces(c["M"], c["N"], seed=c["seed"])
    if c.get("carrier"):
        X += (c["carrier"] * (1 - 2 * (np.arange(c["N"]) % 2))).astype(X.dtype)[None, :]
    if c["M"] >= 3:
        X[c["M"] // 3] = 0                     # one all-zero trace everywhere
    if c.get("holes"):
        punch_holes(X)
    return X.astype(np.float64) if c["f64"] else X


_refs = {}


def reference_of(c, p):
    key = (tuple(sorted(c["kw"].items())), c["M"], c["N"], c["seed"], bool(c.get("holes")), c.get("rows"))
    if key not in _refs:
        # (float64 rows made from float32 ones hold the same values: one reference serves both)
        _refs[key] = reference_planes(p, c["N"], rows_of(c), holes=bool(c.get("holes")))
    return _refs[key]


# ----------------------------------------------------------------------------------------------------------------------------------- route --
def route_of(tp, pl, M, N, tables):
    """What the library says about the call, and the documented size rule of the trace-lane path (include/tspws_hip.h, forward.hip)."""
    lib = tp.load()
    S = pl.S
    sweeps = tp.LIB_PATH.endswith("_sweeps.so")
    sf = lib.tspws_hip_spectral_choice(pl.h, M)
    se = lib.tspws_hip_spectral_end_scale(pl.h)
    NT = lib.tspws_hip_spectral_transform_length(pl.h)
    V = pl.info.V
    forced = os.environ.get("TSPWS_TL_MIN") if sweeps else None
    if sf < S:
        many = True
    elif forced:
        many = M >= max(1, int(forced))
    else:
        many = V > 2 and M >= 128 and M * N >= 7 * 2 ** 20
    blocks = (M + 63) // 64
    pick = 0 if (blocks >= 12 and V > 2) else 1
    if sweeps and os.environ.get("TSPWS_TL_PICK") is not None:
        pick = 1 if int(os.environ["TSPWS_TL_PICK"]) else 0
    r = dict(S=S, spec_first=sf, spec_end=se if sf < S else S, NT=NT, many=many, blocks=blocks, last=M - 64 * (blocks - 1), pick=pick, V=V)
    D = tables["D"]
    if sf < S:
        r["text"] = f"spectral[{sf},{se}) D>={int(D[sf])} NT={NT} + tl[0,{sf}) + gemm[{se},{S}) {blocks} blk"
    elif many:
        r["text"] = f"fir tl[{pick}] {blocks} blk last {r['last']}"
    else:
        r["text"] = f"few-trace M={M}" + (" (1 slice)" if M <= 3 else " (>= 2 slices)" if M > 32 else "")
    return r


def assert_route(c, r, pl, tables):
    e = c["expect"]
    D, S = tables["D"], pl.S
    what = (name_of(c), r["text"])
    if e["path"] == "spectral":
        sf, se = r["spec_first"], r["spec_end"]
        assert sf < se <= S and r["many"], what
        assert all(int(D[s]) >= 8 and int(D[s]) & (int(D[s]) - 1) == 0 for s in range(sf, se)), what
        if "dmin" in e:     # the default rule: octaves of at most max(512, ceil(N / dmin)) outputs, i.e. D >= dmin and, on short traces, finer ones too
            nsmax, Ns = max(512, -(-c["N"] // e["dmin"])), tables["Ns"]
            assert int(Ns[sf]) <= nsmax and (sf == 0 or int(Ns[sf - 1]) > nsmax or int(D[sf - 1]) < 8), what
            assert int(D[sf]) <= e["dmin"], what
        if "dfirst" in e:
            assert int(D[sf]) == e["dfirst"] and (sf == 0 or int(D[sf - 1]) < e["dfirst"]), what
        if "gemm" in e:
            assert S - se == e["gemm"], what
        if "NT" in e:
            assert r["NT"] == e["NT"], what
        if e.get("pow2") is False:
            assert c["N"] & (c["N"] - 1) and r["NT"] >= c["N"] + int(tables["L"][se - 1]) - 1, what
    elif e["path"] == "tl":
        assert r["spec_first"] == S and r["many"], what
        if "pick" in e:
            assert r["pick"] == e["pick"], what
        if "blocks" in e:
            assert r["blocks"] == e["blocks"], what
    elif e["path"] == "few":
        assert r["spec_first"] == S and not r["many"], what
        if "batches" in e:      # (npart >= ncoef: at most budget / (ncoef * 16) traces per batch)
            mb = int(os.environ["TSPWS_PART_MB"])
            per = max(2, ((mb << 20) // (pl.ncoef * 16)) & ~1)
            assert -(-c["M"] // per) >= e["batches"], what
    elif e["path"] == "forced":   # TSPWS_TL_MIN: the many-trace path, with whichever engine the size rule picks
        assert r["many"], what
    else:
        raise AssertionError(e)
    if "last" in e:
        assert r["last"] == e["last"], what
    if "V" in e:
        assert r["V"] == e["V"], what


# ------------------------------------------------------------------------------------------------------------------------------------- run --
def report(line):
    print(line, flush=True)
    path = os.environ.get("TSPWS_PLANES_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def device_rows(X, pad=0):
    import torch
    if not pad:
        return torch.as_tensor(X, device="cuda")
    buf = torch.zeros((X.shape[0], X.shape[1] + pad), dtype=torch.as_tensor(X[:1]).dtype, device="cuda")
    buf[:, : X.shape[1]] = torch.as_tensor(X, device="cuda")
    return buf[:, : X.shape[1]]


def run_case(tp, c, group="default"):
    """One case on the module `tp` (the binding over the shipped or the sweeps library).  Raises on a wrong route or a coefficient outside its bound."""
    N, M = c["N"], c["M"]
    p = tp.resolve(abi.default_params(**c["kw"]), N)
    pl = tp.Plan(p, N)
    tables = pl.tables()
    r = route_of(tp, pl, M, N, tables)
    if c.get("exact"):
        return run_exact(tp, c, pl, r, group)
    assert_route(c, r, pl, tables)
    X = rows_of(c)
    ST, PS = pl.stacks(device_rows(X))
    ref = reference_of(c, abi.resolve(abi.default_params(**c["kw"]), N))
    assert ref.ST.size == pl.ncoef and np.array_equal(ref.D, tables["D"].astype(np.int64)) and np.array_equal(ref.Ns, tables["Ns"].astype(np.int64))
    try:
        w = check_planes(ST, PS, ref, r)
    except AssertionError as err:
        report(f"STACK_PLANES_FAIL {group}: {name_of(c)} | {r['text']} | {err}")
        raise
    assert w["rST"] <= 1 and w["rPS"] <= 1 and ref.max_bPS < ref.cap
    report(f"STACK_PLANES {group}: {name_of(c)} | {r['text']} | max_bPS {ref.max_bPS:.2e} (cap {ref.cap:g}) | dST/bST {w['rST']:.3g} @ scale {w['sST']} | "
           f"dPS/bPS {w['rPS']:.3g} @ scale {w['sPS']}")
    return w


def run_exact(tp, c, pl, r, group):
    """Properties that need no tolerance: the same call twice and the same rows with a padded stride (ld = N + 5) give bit-identical planes;
    an all-zero ensemble gives all-zero planes."""
    X = rows_of(dict(c, holes=False, rows=None))
    a = pl.stacks(device_rows(X))
    b = pl.stacks(device_rows(X))
    d = pl.stacks(device_rows(X, pad=5))
    z = pl.stacks(device_rows(np.zeros_like(X)))
    assert not np.isnan(a[0]).any() and not np.isnan(a[1]).any(), name_of(c)
    for other, what in ((b, "the same call twice"), (d, "rows with a padded stride")):
        assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes(), (name_of(c), r["text"], what)
    assert not z[0].any() and not z[1].any(), (name_of(c), r["text"], "all-zero ensemble")
    report(f"STACK_PLANES {group}: {name_of(c)} | {r['text']} | twice / padded stride bit-identical, all-zero ensemble -> zero planes")


def main(group):
    env, sweeps, _, cases = GROUPS[group]
    for k, v in env.items():
        assert os.environ.get(k) == v, f"the parent sets {k}={v}"
    tp = importlib.import_module("ts-pws_amd")
    assert tp.LIB_PATH.endswith("_sweeps.so") == sweeps, tp.LIB_PATH
    assert tp.load().tspws_hip_device_count() > 0
    ok = bad = 0
    for c in cases:
        try:
            run_case(tp, c, group)
            ok += 1
        except AssertionError as err:
            bad += 1
            print(f"STACK_PLANES_ASSERT {group}: {name_of(c)}: {err}", flush=True)
    print(f"STACK_PLANES_DONE {group} {ok} {bad}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
