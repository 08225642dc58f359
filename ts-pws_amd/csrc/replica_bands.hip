// replica_bands.hip -- percentile bands over replica rows (tspws_hip_replica_bands): per sample, Q quantiles over the replicas of each of B
// ensembles, on the output layout every batched resampling call shares ([B][M][ld] float rows on the device, [B][M] counts on the host).
//
// The order statistic is exact: a float becomes the order-preserving integer key of its bits (negative values: all bits flipped, the others:
// the sign bit set), the k-th smallest key of a column is the largest t with #{key < t} <= k, and t is built bit by bit from bit 31 down --
// one pass over the column per bit, no sort, nothing indexed at run time in registers.  The quantile is the "linear" (type 7) one,
// h = (n - 1) q, j = floor(h), g = h - j: x_(j) when g == 0, else x_(j) + g (x_(j+1) - x_(j)) in FP64 with every operation rounded on its
// own.  x_(j+1) needs no 32 passes of its own: it is x_(j) when #{key <= x_(j)} >= j + 2 (a tie), else the smallest key above x_(j), both
// from ONE further pass.
//   host       per round ONE table block and one upload: the ensembles (first row, participating rows n, offset of their list), the lists of
//              participating rows (h_mtr > 0, or all), j and g of every (ensemble, q); rounds of whole ensembles
//   k_rb_select<QG, false>  (tile of 64 samples x ensemble; one wave) M <= RB_LDS_ROWS: the participating rows of the tile are read from HBM
//              ONCE, coalesced along the samples, and staged in LDS as keys [row][lane] -- lane l walks bank l mod 32 of every row, the two
//              halves of a wave are served in turn: no conflict; then, per group of QG quantiles, 33 passes over the lane's own column
//   k_rb_select<QG, true>   M above that: the same selection with the column read from global memory in every pass (the tile's rows stay in L2)
// A lane reads only what it staged itself, so the kernel has no barrier.  Nothing is atomic, every output has one writer: a repeated call
// is bit-identical.  Columns N .. ld-1 of the rows are never read (the lanes of a partial tile past N read sample N - 1 and store nothing).
#include "tspws_internal.h"
#include "batch_host.h"

enum { RB_TILE = 64, RB_LDS_ROWS = 160 * 1024 / (RB_TILE * 4), RB_QMAX = 8 }; // 640 rows of 64 keys: the 160 KiB a workgroup may declare

// ensemble of a round: index of its first row in d_rows (b M), participating rows, offset of their list, index in the call
struct RbEns { unsigned long long row0; unsigned n, b; unsigned long long list_off; };
// quantile of an ensemble: x_(j) + g (x_(j+1) - x_(j))
struct RbQ { double g; unsigned j, pad; };

__device__ __forceinline__ unsigned rb_key(const float v)
{
	const unsigned u = __float_as_uint(v);
	return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float rb_value(const unsigned k)
{
	return __uint_as_float(k ^ ((unsigned)((int)~k >> 31) | 0x80000000u));
}

extern __shared__ unsigned rb_keys[]; // [n][RB_TILE]

// bands[e.b][q][s] for the samples s of tile blockIdx.x and the ensemble e = ens[blockIdx.y] of the round, QG quantiles per group of passes
// (the groups share the staged tile).  list[e.list_off + i] = the i-th participating row of the ensemble, qt[blockIdx.y Q + q] its j and g.
template <int QG, bool GLOBAL>
__global__ void __launch_bounds__(RB_TILE) k_rb_select(const float *__restrict__ rows, size_t ld, size_t N, const RbEns *__restrict__ ens,
                                                        const unsigned *__restrict__ list, const RbQ *__restrict__ qt, unsigned Q, float *__restrict__ bands)
{
#pragma clang fp contract(off) // g (x1 - x0) is rounded before it is added
	const unsigned lane = threadIdx.x;
	const size_t s = (size_t)blockIdx.x * RB_TILE + lane;
	const bool live = s < N;
	const RbEns e = ens[blockIdx.y];
	const unsigned n = e.n;
	const unsigned *rl = list + e.list_off;
	const RbQ *eq = qt + (size_t)blockIdx.y * Q;
	float *o = bands + (size_t)e.b * Q * N + s;
	if (!n) { // no replica takes part: zero bands
		if (live) for (unsigned q = 0; q < Q; q++) o[(size_t)q * N] = 0.f;
		return;
	}
	const float *col = rows + e.row0 * ld + (live ? s : N - 1);
	if (!GLOBAL) { // eight rows' loads in flight
		for (unsigned i0 = 0; i0 < n; i0 += 8) {
			float v[8];
#pragma unroll
			for (int u = 0; u < 8; u++) v[u] = col[(size_t)rl[i0 + (unsigned)u < n ? i0 + (unsigned)u : n - 1] * ld];
#pragma unroll
			for (int u = 0; u < 8; u++)
				if (i0 + (unsigned)u < n) rb_keys[(i0 + (unsigned)u) * RB_TILE + lane] = rb_key(v[u]);
		}
	}
	auto key_of = [&](const unsigned i) -> unsigned { return GLOBAL ? rb_key(col[(size_t)rl[i] * ld]) : rb_keys[i * RB_TILE + lane]; };

	for (unsigned q0 = 0; q0 < Q; q0 += QG) { // (slots past Q repeat the last quantile and store nothing)
		unsigned j[QG], t[QG];
#pragma unroll
		for (int k = 0; k < QG; k++) { j[k] = eq[q0 + (unsigned)k < Q ? q0 + (unsigned)k : Q - 1].j; t[k] = 0; }
		for (int bit = 31; bit >= 0; bit--) {
			unsigned cand[QG], cnt[QG];
#pragma unroll
			for (int k = 0; k < QG; k++) { cand[k] = t[k] | (1u << bit); cnt[k] = 0; }
#pragma unroll 4
			for (unsigned i = 0; i < n; i++) {
				const unsigned key = key_of(i);
#pragma unroll
				for (int k = 0; k < QG; k++) cnt[k] += key < cand[k];
			}
#pragma unroll
			for (int k = 0; k < QG; k++) t[k] = cnt[k] <= j[k] ? cand[k] : t[k];
		}
		// t = x_(j); its successor: x_(j) again when the tie reaches rank j + 1, else the smallest key above it
		unsigned le[QG], up[QG];
#pragma unroll
		for (int k = 0; k < QG; k++) { le[k] = 0; up[k] = 0xffffffffu; }
#pragma unroll 4
		for (unsigned i = 0; i < n; i++) {
			const unsigned key = key_of(i);
#pragma unroll
			for (int k = 0; k < QG; k++) {
				le[k] += key <= t[k];
				up[k] = (key > t[k] && key < up[k]) ? key : up[k];
			}
		}
#pragma unroll
		for (int k = 0; k < QG; k++) {
			if (q0 + (unsigned)k < Q && live) {
				const double g = eq[q0 + (unsigned)k].g;
				const float x0 = rb_value(t[k]);
				float r = x0;
				if (g != 0.) { // (then j + 1 <= n - 1)
					const float x1 = rb_value(le[k] >= j[k] + 2u ? t[k] : up[k]);
					r = (float)((double)x0 + g * ((double)x1 - (double)x0));
				}
				o[(size_t)(q0 + (unsigned)k) * N] = r;
			}
		}
	}
}

namespace {

// the tables of a round in one block: ensembles | j and g of every (ensemble, q) | lists of participating rows
struct RbTab { size_t ens, qt, list, bytes; };
RbTab rb_tab(size_t ne, size_t nq, size_t nlist)
{
	TableLayout lay;
	const size_t ens = lay.add<RbEns>(ne), qt = lay.add<RbQ>(nq), list = lay.add<unsigned>(nlist);
	return {ens, qt, list, lay.bytes};
}

template <int QG>
int launch(bool global, dim3 grid, size_t lds, hipStream_t st, const float *rows, size_t ld, size_t N, const RbEns *ens, const unsigned *list, const RbQ *qt,
           unsigned Q, float *bands)
{
	if (global) {
		hipLaunchKernelGGL((k_rb_select<QG, true>), grid, dim3(RB_TILE), 0, st, rows, ld, N, ens, list, qt, Q, bands);
		return 0;
	}
	if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)k_rb_select<QG, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); // (per device: every launch)
	hipLaunchKernelGGL((k_rb_select<QG, false>), grid, dim3(RB_TILE), lds, st, rows, ld, N, ens, list, qt, Q, bands);
	return 0;
}

} // namespace

extern "C" int tspws_hip_replica_bands(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const double *h_q,
                                       unsigned Q, float *d_bands, void *s)
{
	// first what needs no plan
	if (Q > RB_QMAX) return fail(TSPWS_E_ARG, "replica_bands: more than 8 quantiles in one call");
	if (!B || !M || !Q) return pl ? 0 : fail(TSPWS_E_ARG, "replica_bands: NULL");
	if (!d_rows || !h_q || !d_bands) return fail(TSPWS_E_ARG, "replica_bands: NULL");
	for (unsigned q = 0; q < Q; q++)
		if (!(h_q[q] >= 0. && h_q[q] <= 1.)) return fail(TSPWS_E_ARG, "replica_bands: a probability outside [0, 1]"); // (NaN included)
	if (!pl) return fail(TSPWS_E_ARG, "replica_bands: NULL");
	if (ld < pl->N) return fail(TSPWS_E_ARG, "replica_bands: row stride below the trace length");

	const size_t N = pl->N, budget = tspws_part_budget_bytes();
	const bool global = M > RB_LDS_ROWS; // the route: by M alone
	// participating rows in front of ensemble b
	std::vector<size_t> n0((size_t)B + 1, 0);
	for (unsigned b = 0; b < B; b++) {
		size_t n = M;
		if (h_mtr) { n = 0; for (unsigned m = 0; m < M; m++) n += h_mtr[(size_t)b * M + m] > 0; }
		n0[b + 1] = n0[b] + n;
	}
	// rounds of whole ensembles: ensembles within grid.y, the rows a round reads and its tables within the budget
	auto tab_of = [&](size_t j0, size_t j1) { return rb_tab(j1 - j0, (j1 - j0) * Q, n0[j1] - n0[j0]); };
	const std::vector<Round> rounds = whole_ensemble_rounds(B, [&](size_t j0, size_t j1) {
		const size_t ne = j1 - j0;
		return !(ne > 65535 || ne * M * ld * sizeof(float) + tab_of(j0, j1).bytes > budget);
	});
	size_t max_tab = 0;
	for (const Round &r : rounds) max_tab = std::max(max_tab, tab_of(r.j0, r.j1).bytes);
	const unsigned QG = (Q + (Q + 3) / 4 - 1) / ((Q + 3) / 4); // quantiles per group of passes: Q in one group up to 4, else two even groups
	const size_t tiles = (N + RB_TILE - 1) / RB_TILE;

	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_bands_stats &stats = pl->bands_stats;
	stats = tspws_hip_bands_stats();
	stats.lds_max_rows = RB_LDS_ROWS;
	BatchCall call(st);
	int rc;
	for (const Round &r : rounds) {
		const size_t ne = r.j1 - r.j0;
		stats.rounds++;
		const RbTab o = tab_of(r.j0, r.j1);
		char *blob = call.block(o.bytes), *tab;
		RbEns *he = (RbEns *)(blob + o.ens);
		RbQ *hq = (RbQ *)(blob + o.qt);
		unsigned *hl = (unsigned *)(blob + o.list);
		size_t nmax = 0;
		for (size_t b = r.j0; b < r.j1; b++) {
			const size_t n = n0[b + 1] - n0[b], off = n0[b] - n0[r.j0];
			RbEns d;
			d.row0 = (unsigned long long)b * M; d.n = (unsigned)n; d.b = (unsigned)b; d.list_off = off;
			he[b - r.j0] = d;
			unsigned *l = hl + off;
			for (unsigned m = 0; m < M; m++)
				if (!h_mtr || h_mtr[b * M + m] > 0) *l++ = m;
			for (unsigned q = 0; q < Q; q++) {
				RbQ &e = hq[(b - r.j0) * Q + q];
				const double h = n ? (double)(n - 1) * h_q[q] : 0., j = floor(h);
				e.j = (unsigned)j; e.g = h - j; e.pad = 0;
			}
			nmax = std::max(nmax, n);
			if (!n) stats.empty++; else if (global) stats.global++; else stats.lds++;
		}
		if ((rc = call.upload(pl, SCR_RBTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const dim3 grid((unsigned)tiles, (unsigned)ne);
		const size_t lds = global ? 0 : nmax * RB_TILE * sizeof(unsigned);
		const float *rows = d_rows;
		const RbEns *d_ens = (const RbEns *)(tab + o.ens);
		const RbQ *d_qt = (const RbQ *)(tab + o.qt);
		const unsigned *d_list = (const unsigned *)(tab + o.list);
		switch (QG) {
		case 1: rc = launch<1>(global, grid, lds, st, rows, ld, N, d_ens, d_list, d_qt, Q, d_bands); break;
		case 2: rc = launch<2>(global, grid, lds, st, rows, ld, N, d_ens, d_list, d_qt, Q, d_bands); break;
		case 3: rc = launch<3>(global, grid, lds, st, rows, ld, N, d_ens, d_list, d_qt, Q, d_bands); break;
		default: rc = launch<4>(global, grid, lds, st, rows, ld, N, d_ens, d_list, d_qt, Q, d_bands); break;
		}
		if (rc) return rc;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // bands complete
	return 0;
}

extern "C" int tspws_hip_replica_bands_stats(const tspws_hip_plan *pl, tspws_hip_bands_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "replica_bands_stats: NULL");
	*stats = pl->bands_stats;
	stats->lds_max_rows = RB_LDS_ROWS;
	return 0;
}
