"""The host plan of the dynamic time warping call against a direct enumeration, on the CPU: `make -C ts-pws_amd dtw_plan_check` builds
tests/dtw_plan_check.cpp -- a stand-alone program over csrc/dtw_plan.h, which holds no HIP -- with AddressSanitizer + UBSan, and this test
runs it as a child process.  No GPU and no library needed.

The program requires that the parameter and range checks refuse exactly what lies outside the contract's ranges, each limit from both sides;
that the lags per lane, the samples T, the per-range offsets and the choice-plane sizes are what a sample-by-sample enumeration gives, every
(sample, lag) owning its own two bits inside its range's plane, a range alone giving the same sizes; that the wave's LDS holds its rings, its
two staged chunks and its backtrack block; that the rounds keep within the budget unless they are one ensemble, and are maximal; and that
the table block (allocated at its exact size) numbers the participating rows in order.  N = 1501, Lmax in {1, 31, 32, 127}, b in {1, 8}."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "dtw_plan_check")


def test_plan_matches_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "dtw_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
