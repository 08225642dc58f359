"""What the host plans share against a direct enumeration, on the CPU: `make -C ts-pws_amd host_plan_check` builds
tests/host_plan_check.cpp -- a stand-alone program over csrc/host_plan.h, which holds no HIP -- with AddressSanitizer + UBSan, and this test
runs it as a child process.  No GPU and no library needed.

The program requires that a table layout aligns every array behind the one before; that the rounds of whole ensembles tile the list in
order, keep within the budget unless they are one ensemble, and are maximal; that participating_rows0 counts and both slot fillers number
exactly the participating rows in order, the others getting NOSLOT, with every callback seen once (h_mtr NULL, all zero and mixed; arrays of
their exact size); that largest_fitting returns the largest count that fits, and 1 when none does; that the task packer tiles the items,
respects the pass limit, is maximal and never crosses a forced restart; and that the range checks accept and refuse each limit from both
sides with the words of the list they are given.  B up to 5, M up to 4, up to 40 items."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "host_plan_check")


def test_shared_helpers_match_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "host_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
