"""The checker of the percentile bands over replica rows (tspws_hip_replica_bands, Plan.replica_bands), numpy only: per ensemble np.sort
along the replica axis of the participating rows, then the "linear" (type 7) quantile exactly as include/tspws_hip.h states it -- for n
participating replicas and probability q: h = (double)(n - 1) * q, j = floor(h), g = h - j; the band is (float) x_(j) when g == 0, else
(float)((double) x_(j) + g * ((double) x_(j+1) - (double) x_(j))), every FP64 operation rounded on its own (numpy fuses nothing).  n = 0
gives zero bands.  For finite values and infinities np.sort's order is the order of the definition's integer key up to the sign of zero."""
import numpy as np


def expected(rows, q, mtr=None):
    """bands float32 [B][Q][N] of rows float32 [B][M][N] (columns past N already cut), probabilities q, counts mtr (None or [B][M])."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 3
    q = np.asarray(q, dtype=np.float64)
    B, M, N = rows.shape
    out = np.zeros((B, q.size, N), np.float32)
    for b in range(B):
        take = np.ones(M, bool) if mtr is None else np.asarray(mtr)[b] > 0
        n = int(take.sum())
        if not n:
            continue
        x = np.sort(rows[b][take], axis=0).astype(np.float64)
        for k in range(q.size):
            h = np.float64(n - 1) * q[k]
            j = int(np.floor(h))
            g = h - np.float64(j)
            if g == 0:
                out[b, k] = x[j].astype(np.float32)
            else:
                with np.errstate(invalid="ignore"):  # inf - inf: NaN, as on the device
                    out[b, k] = (x[j] + g * (x[j + 1] - x[j])).astype(np.float32)
    return out


def parity_rows(B, M, N, ld, seed):
    """The parity batch as a [B][M][ld] base: seeded normals times a per-column scale of 1e-6 .. 1e2, a constant column, a tie column
    (small integers), a +-0 column, one +inf and one -inf entry; the pad columns N .. ld-1 hold NaN."""
    rng = np.random.default_rng(seed)
    base = np.full((B, M, ld), np.nan, np.float32)
    scale = (10.0 ** rng.uniform(-6, 2, N)).astype(np.float32)
    x = rng.standard_normal((B, M, N)).astype(np.float32) * scale
    x[:, :, 3] = 2.5
    x[:, :, 5] = rng.integers(-3, 4, (B, M)).astype(np.float32)
    x[:, :, 7] = np.where(rng.integers(0, 2, (B, M)) == 1, np.float32(-0.0), np.float32(0.0))
    x[0, 0, 11] = np.inf
    x[B - 1, M - 1, 13] = -np.inf
    base[:, :, :N] = x
    return base


def parity_counts(B, M, seed):
    """A count table [B][M] for the parity batch: ensemble 1 has every row 0, ensemble 2 exactly one row > 0, the others a few rows 0."""
    rng = np.random.default_rng(seed)
    mtr = rng.integers(1, 500, (B, M)).astype(np.uint32)
    for b in range(B):
        if M > 2:
            mtr[b, rng.choice(M, size=max(1, M // 5), replace=False)] = 0
    mtr[1] = 0
    mtr[2] = 0
    mtr[2, M // 2] = 3
    return mtr
