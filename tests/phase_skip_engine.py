"""Child process of tests/test_phase_skip_gpu.py: whole tspws_main calls on wide-dynamic-range ensembles (abi.wide_traces) with the forward
engine pinned by TSPWS_ENGINE (read once per process by the library), against the FP64 FIR oracle.  argv[1] names the pin the parent set.
Prints PHASE_SKIP <case> <relerr> per case, then PHASE_SKIP_DONE <worst> <digest of all float outputs>; exits 1 on a case over 2e-6."""
import hashlib
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import abi

tspws = importlib.import_module("ts-pws_amd")
lib = tspws.load()
engine = sys.argv[1]
assert os.environ.get("TSPWS_ENGINE") == engine
worst, bad = 0.0, []
h = hashlib.sha1()


def check(name, kw, mtr, N, seed, rows):
    """rows: the count of traces / partial-stack rows the forward engine sees (mtr, or Kmax of a two-stage call)."""
    global worst
    p = abi.default_params(**kw)
    pl = tspws.Plan(tspws.resolve(p, N), N)
    choice = lib.tspws_hip_spectral_choice(pl.h, rows)
    if engine == "fir":
        assert choice == pl.S, (name, choice)                # no spectral set whatever the size
    else:
        assert choice < pl.S, (name, choice)                 # pinned: even a small batch goes through the spectrum
    X = abi.wide_traces(mtr, N, seed=seed, every=max(1, mtr // 12))
    a = abi.run_main(lib.tspws_main, p, X)
    b = abi.run_main(abi.oracle().orc_tspws_main, p, X)
    assert a["rc"] == 0 and b["rc"] == 0, (name, a["rc"], b["rc"])
    e = max(abi.relerr(a["ls"], b["ls"]), abi.relerr(a["tsPWS"], b["tsPWS"]))
    print("PHASE_SKIP", name, f"{e:.3e}", flush=True)
    worst = max(worst, e)
    if not e < 2e-6:
        bad.append(name)
    h.update(a["ls"].tobytes()); h.update(a["tsPWS"].tobytes())


if engine == "fir":
    # >= 128 traces and >= 7 M samples with more than two voices per octave: the trace-lane kernel k_fwd_tl takes every scale
    check("fir_trace_lane_128x57344", dict(), 128, 57344, 21, 128)
    check("fir_few_trace_256x4096_exact_morlet", dict(type=-2), 256, 4096, 22, 256)
else:
    check("spectral_100x4096", dict(), 100, 4096, 23, 100)
    check("spectral_rows_k70_unbiased_wu15", dict(Kmax=70, unbiased=1, wu=1.5), 70, 4096, 24, 70)
    check("spectral_mexhat_80x4097", dict(type=-3), 80, 4097, 25, 80)
print("PHASE_SKIP_DONE", worst, h.hexdigest()[:16], flush=True)
sys.exit(1 if bad else 0)
