"""The host plan of the moving-window cross-spectrum call against a direct enumeration, on the CPU: `make -C ts-pws_amd
mwcs_plan_check` builds tests/mwcs_plan_check.cpp -- a stand-alone program over csrc/mwcs_plan.h, which holds no HIP -- with AddressSanitizer +
UBSan, and this test runs it as a child process.  No GPU and no library needed.

The program requires that the parameter check refuses exactly what lies outside the contract's ranges, each limit from both sides, and
more than 64 bins with the smoothing margins; that the bins, the padded table sizes and the basis layout are what the contract states, Tc and
Ts the ascending-l sums of the entries; that a start belongs to a lag range iff the definition says so, decided start by start, the list
holding exactly those, range after range, and a range alone giving the same windows; that the rounds keep within the budget unless they are
one ensemble, and are maximal; and that the table block (allocated at its exact size) holds every array inside it, aligned for the kernel's
32-byte loads, the transposed basis zero past L and past 2 Qx columns, the sources and the slots agreeing with the participation rule.
L = 16 .. 1024, hops 1 .. L, range edges at and around L and the trace ends; N = 1501."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "mwcs_plan_check")


def test_plan_matches_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "mwcs_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
