"""The host tables of the two-stage replicas against their per-trace definition, on the CPU: `make -C ts-pws_amd column_runs_check` builds
tests/column_runs_check.cpp -- a stand-alone program over csrc/column_runs.h and csrc/masked_tables.h, which hold no HIP -- with
AddressSanitizer + UBSan, and this test runs it as a child process.  No GPU and no library needed.

The program computes the group of every trace in every column trace by trace (replica: floor(k Kmax / max(K_c, 1)), k = rank among the
bytes == 1, any other byte deleted; plain stack: min(floor(i Kmax / m), Kmax - 1)), gives every trace a random 64-bit integer and simulates
each table form in wrap-around integer arithmetic by its kernel's contract: the direct walk with its two segments per stage and fix rows, the
snapshot form with segments, carries and signed terms, and the batch's walk per (ensemble, tile of 16 columns).  It requires: every run has
one signature in every column, the runs tile the shard in order and none is empty, every row equals the sum of the traces of its (column,
group) -- a stage's rows as soon as the stage is walked --, the rows never stored are exactly those without a trace, `unwritten` says
whether there is one, fix_row is the first row a column stores at or after the stage's middle, Kc and Mv are the byte counts, and the
block holds every array at its offset with the 16-byte records aligned.

Grid (seeded): m in 1, 2, 7, 8, 9, 63, 64, 65, 70, 257; Kmax in 1, 2, 3, 10, m + 3; W in 1, 15, 16, 17, 33 (with and without the plain
stack); groups per stage 1, 3, Kmax; shards whole, empty and three partial ones (the program counts those whose edges fall inside a run and
inside a kept stretch of >= 8 bytes); the direct form allowed and not; N in 1000, 4096, 87000 (N only sets the segment count).  Columns
cycle through: all kept, all deleted, fewer kept than groups, alternating, one kept stretch of 8 / 9 / 17 bytes at offsets 0..7, bytes 2 and
-1 mixed in, random."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "ts-pws_amd")
BIN = os.path.join(PKG, "bin", "column_runs_check")


def test_run_tables_match_the_per_trace_definition():
    r = subprocess.run(["make", "-C", PKG, "column_runs_check"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(BIN), r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    bad = [l for l in out.splitlines() if "AddressSanitizer" in l or "LeakSanitizer" in l or "runtime error" in l]
    assert r.returncode == 0 and not bad and "agree with the per-trace definition" in r.stdout, (r.returncode, out[-3000:])
