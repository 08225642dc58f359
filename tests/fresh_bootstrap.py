"""Run by test_bootstrap_batch_cpu.py in a FRESH process per seed (argv[1]): the host draws of the bootstrap (tspws_bootstrap_plan,
tspws_bootstrap_plan_batch) against a Python restatement driven by libc rand() through ctypes from the same srand -- every row of an ensemble
sums to its trace count, the batch draws in the order of a loop over ensembles and replicas, empty ensembles draw nothing, and the calls that
return 1 write nothing and leave the rand() state alone.  Prints FRESH_BOOTSTRAP OK <seed>; any failed check ends it with a traceback."""
import ctypes as C
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import abi

tspws = importlib.import_module("ts-pws_amd")
lib = tspws.load()
libc = C.CDLL(None)
RAND_MAX = 2147483647  # glibc
seed = int(sys.argv[1])
SIZES, M, first0 = [0, 1, 5, 64, 0, 300], 4, 3
first = np.concatenate([[first0], first0 + np.cumsum(SIZES)]).astype(np.uint64)
T = int(first[-1] - first[0])


def draw(J):
    """tspws_bootstrap_plan restated: J draws with replacement, a draw on a full count drawn again."""
    cnt = np.zeros(J, np.uint8)
    d = 0
    while d < J:
        i = int(libc.rand() * (float(J) / (float(RAND_MAX) + 1.0)))
        if cnt[i] == 255:
            continue
        cnt[i] += 1
        d += 1
    return cnt


def state():
    """The generator's next value: equal after equal numbers of draws from one seed.  (It consumes a value: callers re-seed.)"""
    return libc.rand()


# the batch against the restatement, draw for draw
got = np.full((M, T), 7, np.uint8)
abi.srand(seed)
assert lib.tspws_bootstrap_plan_batch(got.ctypes.data, first.ctypes.data, len(SIZES), M) == 0
after = state()
want = np.full((M, T), 7, np.uint8)
abi.srand(seed)
for b, mb in enumerate(SIZES):
    c0 = int(first[b] - first[0])
    for m in range(M):
        if mb:
            want[m, c0:c0 + mb] = draw(mb)
assert state() == after, "another number of draws"
np.testing.assert_array_equal(got, want)
for b, mb in enumerate(SIZES):
    c0 = int(first[b] - first[0])
    assert (got[:, c0:c0 + mb].astype(np.int64).sum(axis=1) == mb).all(), b  # every row of an ensemble sums to M_b
assert got.max() > 1 and got.min() == 0  # (with replacement)

# ... against a loop of single draws over ensembles and replicas
loop = np.full((M, T), 7, np.uint8)
abi.srand(seed)
for b, mb in enumerate(SIZES):
    c0 = int(first[b] - first[0])
    for m in range(M):
        row = np.full(mb + 1, 9, np.uint8)
        assert lib.tspws_bootstrap_plan(row.ctypes.data, mb) == 0
        assert row[mb] == 9
        loop[m, c0:c0 + mb] = row[:mb]
assert state() == after
np.testing.assert_array_equal(loop, want)

# ... and through the binding
abi.srand(seed)
np.testing.assert_array_equal(tspws.bootstrap_counts_batch(first, M), want)
assert state() == after

# empty ensembles and J == 0 draw nothing
abi.srand(seed)
r0 = state()
abi.srand(seed)
empty = np.array([5, 5, 5, 5], dtype=np.uint64)
one = np.full(4, 9, np.uint8)
assert lib.tspws_bootstrap_plan_batch(one.ctypes.data, empty.ctypes.data, 3, 6) == 0
assert lib.tspws_bootstrap_plan(one.ctypes.data, 0) == 0
assert tspws.bootstrap_counts_batch([3, 3], 2).shape == (2, 0)
assert (one == 9).all() and state() == r0

# the calls that return 1 write nothing and leave the rand() state alone
abi.srand(seed)
cnt = np.full((2, 9), 7, np.uint8)
ok = np.array([0, 5, 9], dtype=np.uint64)
bad = np.array([0, 5, 4], dtype=np.uint64)
assert lib.tspws_bootstrap_plan(None, 5) == 1
assert lib.tspws_bootstrap_plan_batch(None, ok.ctypes.data, 2, 2) == 1
assert lib.tspws_bootstrap_plan_batch(cnt.ctypes.data, None, 2, 2) == 1
assert lib.tspws_bootstrap_plan_batch(cnt.ctypes.data, bad.ctypes.data, 2, 2) == 1
assert (cnt == 7).all() and state() == r0
try:
    tspws.bootstrap_counts_batch([0, 5, 4], 2)
    raise SystemExit("decreasing offsets accepted by the binding")
except tspws.TspwsError:
    pass

# (the redraw on a full count cannot be reached with J draws on J traces and a real generator: a count of 256 needs 256 of at least 256 draws
# on one trace; the restatement above states the rule, the counts' type bounds them)
print("FRESH_BOOTSTRAP OK", seed)
