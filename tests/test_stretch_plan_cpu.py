"""The host plan of the stretching call against a direct enumeration, on the CPU: `make -C ts-pws_amd stretch_plan_check` builds
tests/stretch_plan_check.cpp -- a stand-alone program over csrc/stretch_plan.h, which holds no HIP -- with AddressSanitizer + UBSan, and
this test runs it as a child process.  No GPU and no library needed.

The program requires that every (ensemble, stretch, window sample) falls into exactly one round, chunk and segment; that the segments of a
window depend on that window alone and their packed columns tile [0, J) in multiples of 4; that a round's partial sums, table and one chunk
of stretched references stay within the budget unless the round is one ensemble at 16 stretches, and that no round or chunk could have been
larger; and that the table block (allocated at its exact size) holds every array inside it, with the tiles, the row lists and the slots
agreeing with the participation rule.  Grid: B in 1, 2, 3, 7, 40; M in 1 .. 100 around the tile sizes 16 and 32; E in 1, 15, 16, 17, 4096;
one to four windows with edges around the multiples of 4 and of the segment length; all rows, a third left out, none taking part; budgets
from 1 byte to 1 TB around the sizes at which the rounds change."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "stretch_plan_check")


def test_plan_matches_the_direct_enumeration():
    r = subprocess.run(["make", "-C", PKG, "stretch_plan_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the direct enumeration" in r.stdout, (r.returncode, out[-3000:])
