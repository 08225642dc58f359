"""The host plan of the wavelet cross-spectrum calls against a direct per-coefficient enumeration, on the CPU: `make -C ts-pws_amd
wxs_plan_check` builds tests/wxs_plan_check.cpp -- a stand-alone program over csrc/wxs_plan.h, which holds no HIP -- with AddressSanitizer +
UBSan, and this test runs it as a child process.  No GPU and no library needed.

The program requires that the scales in use are exactly those inside a band; that for every (scale in use, window) the coefficients that the
definition lets take part -- window and, under the wrap rule, filter support, decided coefficient by coefficient -- are exactly those of the
span's items, each once; that the items of a span depend on that scale and window alone (the plan of that band and window alone gives the
same ones) and start at multiples of the segment length from the range's first index; that the tasks tile the items within their pass limit
and are maximal; that the rounds and row chunks keep within the budget unless they are one ensemble or one row, and are maximal; and that
the table block (allocated at its exact size) holds every array inside it, the row list and the slots agreeing with the participation rule.
Frames of 15 scales with power-of-two and odd decimations, filters longer than the trace and a negative centre; N = 64, 1025, 1501, 4096."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "wxs_plan_check")


def test_plan_matches_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "wxs_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
