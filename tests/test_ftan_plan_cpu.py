"""The host plan of the group-arrival calls against a direct per-index enumeration, on the CPU: `make -C ts-pws_amd ftan_plan_check` builds
tests/ftan_plan_check.cpp -- a stand-alone program over csrc/ftan_plan.h, which holds no HIP -- with AddressSanitizer + UBSan, and this test
runs it as a child process.  No GPU and no library needed.

The program requires that two ensembles share a class exactly when their window sets (and noise ranges, when noise is wanted) are equal by
value; that for every (class, scale, window) and (class, scale, noise range) the indices that the definition makes members -- window and,
under the wrap rule, filter support, decided index by index -- are exactly those of the span's items, each once, in segments counted from
the first member (the plan of that ensemble, window and scale alone gives the same ones); that the tasks tile each class's items within
their pass limit, are maximal and never cross a class; that the rounds and row chunks keep within the budget unless they are one ensemble or
one row, and are maximal; and that the table block (allocated at its exact size) holds every array inside it, the row list, the classes and
the slots agreeing with the participation rule, every partial entry inside the partial block.  Frames of 15 scales with power-of-two and
odd decimations, filters longer than the trace and a negative centre; N = 64, 1025, 1501, 4096; 1 to 4 windows; 1, 2 and 5 ensembles."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "ftan_plan_check")


def test_plan_matches_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "ftan_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
