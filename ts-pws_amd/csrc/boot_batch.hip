// boot_batch.hip -- bootstrap replicas of many ensembles in one call (tspws_hip_bootstrap_batch, tspws_hip_bootstrap_batch_cnt) and the host draw
// (tspws_bootstrap_plan, tspws_bootstrap_plan_batch).  Reference citations are relative to the reference project's src/ directory.
//
// A bootstrap replica draws M_b traces of an ensemble WITH replacement: a trace enters it 0, 1, 2, .. times, which no 0/1 selection can say.
// Replica (b, m) here is the single-stage resampling body (tspws_subsmpl_float, ts_pws1f_lib.c:501-610) with an all-ones mask on the EXPANDED
// ensemble -- the traces of ensemble b in trace order, trace i repeated cnt[m][i] times -- without ever forming that ensemble: the linear and
// phase stacks are sums over traces, so multiplicity only says how often a trace's coefficient and unit phasor are added.
//   host       K_{b,m} = the counts of row m inside ensemble b
//   rounds     those of row_batch.h with a count byte as a row's code of a trace (CountRows): the 8 counts of a trace in one aligned 8-byte
//              word, a count adds the trace that many times -- repeated addition, the order of operations of the expanded ensemble; at the
//              end of a round k_bt_moments (sample tile x ensemble): mean and standard error over the replicas
// A 0/1 count row runs exactly the arithmetic of a mask row of sub_batch.hip.  Two-stage ensembles are refused: in the expanded ensemble the
// group of a copy is floor(k Kmax / K), so a repeated trace can straddle group borders, which needs a walk of its own.
#include "tspws_internal.h"
#include "row_batch.h"

// mean and bootstrap standard error of the float rows of ensemble blockIdx.y of the round, per sample, over its replicas with K > 0 (n of them):
// stats[b][0 | 1][.] of ls_out, stats[b][2 | 3][.] of ts_out.  Two FP64 passes in replica order, every operation rounded on its own:
// mean = (sum v) / n, error = sqrt((sum (v - mean)^2) / (n - 1)); n <= 1: error 0; n = 0: mean 0.
__global__ void __launch_bounds__(256) k_bt_moments(const float *__restrict__ ls, const float *__restrict__ ts, size_t N, const SbEns *__restrict__ ens,
                                                    const unsigned *__restrict__ Kc, unsigned M, float *__restrict__ stats)
{
#pragma clang fp contract(off) // (v - mean)^2 is rounded before it is added
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned row = ens[blockIdx.y].row;
	const unsigned *kc = Kc + (size_t)blockIdx.y * M;
#pragma unroll
	for (int w = 0; w < 2; w++) {
		const float *src = (w ? ts : ls) + (size_t)row * M * N + n;
		double s = 0;
		unsigned cn = 0;
		for (unsigned m = 0; m < M; m++)
			if (kc[m]) { s += (double)src[(size_t)m * N]; cn++; } // (wave-uniform)
		const double mean = cn ? s / (double)cn : 0.;
		double ss = 0;
		for (unsigned m = 0; m < M; m++)
			if (kc[m]) { const double d = (double)src[(size_t)m * N] - mean; ss += d * d; }
		float *o = stats + ((size_t)row * 4 + 2 * (size_t)w) * N + n;
		o[0] = (float)mean;
		o[N] = cn > 1 ? (float)sqrt(ss / (double)(cn - 1)) : 0.f;
	}
}

// a row's code of a trace: how often the trace enters the replica (replicas past M: zero)
struct CountRows {
	using Entry = unsigned long long;
	using Value = unsigned char;
	struct Codes { unsigned w0, w1; };
	using Lane = unsigned char;
	using Code = unsigned;
	using Rows = KRows;
	using Row = void;
	static constexpr bool CODES_AHEAD = false, LOAD_ALL = true;
	static constexpr unsigned SPARE = 0;
	static constexpr const char *NAME = "bootstrap_batch", *ROWS = "replica rows";
	static constexpr auto launch_weight = launch_sb_weight;
	const Value *h;
	static void put(Entry &e, unsigned lane, Value v) { ((unsigned char *)&e)[lane] = v; }
	static __device__ __forceinline__ Codes fetch(const Entry *t)
	{
		const unsigned long long w = *t;
		return {(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w), (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w >> 32))};
	}
	static __device__ __forceinline__ void add(Codes w, int m, double2 &st, double2 &ps, const double2 &a, const double2 &u)
	{
		const unsigned c = ((m < 4 ? w.w0 : w.w1) >> (8 * (m & 3))) & 255u; // (wave-uniform)
		for (unsigned r = 0; r < c; r++) { st.x += a.x; st.y += a.y; ps.x += u.x; ps.y += u.y; } // one addition per copy
	}
	static __device__ __forceinline__ Code code(Lane x, unsigned) { return x; }
	static __device__ __forceinline__ float add(float acc, Code c, float v)
	{
		for (unsigned r = 0; r < c; r++) acc = (float)((double)acc + (double)v); // one addition per copy
		return acc;
	}
};

namespace {

// what both entries refuse (row_batch_check)
int check_args(const tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M, bool cnt_ok,
               const float *d_ls_out, const float *d_ts_out, const unsigned *h_mtr_out, bool *done)
{
	return row_batch_check(CountRows::NAME, "a two-stage ensemble (0 < Kmax <= its traces): the two-stage bootstrap is not built, only single-stage ensembles", pl, p, d_x, ld,
	                       h_first, B, M, cnt_ok, d_ls_out, d_ts_out, h_mtr_out, done, [] { return 0; });
}

} // namespace

extern "C" int tspws_bootstrap_plan(unsigned char *cnt, size_t J)
{
	if (!cnt) return 1;
	memset(cnt, 0, J);
	const double scale = (double)J / ((double)RAND_MAX + 1.0);
	for (size_t d = 0; d < J;) {
		const size_t i = (size_t)(rand() * scale);
		if (cnt[i] == 255) continue; // a full count: drawn again
		cnt[i]++;
		d++;
	}
	return 0;
}

extern "C" int tspws_bootstrap_plan_batch(unsigned char *cnt, const size_t *first, unsigned B, unsigned M)
{
	if (!cnt || !first) return 1;
	for (unsigned b = 0; b < B; b++) if (first[b + 1] < first[b]) return 1;
	const size_t T = first[B] - first[0];
	for (unsigned b = 0; b < B; b++) {
		const size_t m = first[b + 1] - first[b];
		if (!m) continue;
		for (unsigned q = 0; q < M; q++) tspws_bootstrap_plan(cnt + (size_t)q * T + (first[b] - first[0]), m);
	}
	return 0;
}

extern "C" int tspws_hip_bootstrap_batch_cnt(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                             const unsigned char *h_cnt, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, float *d_stats, void *s)
{
	bool done;
	int rc;
	if ((rc = check_args(pl, p, d_x, ld, h_first, B, M, h_cnt != nullptr, d_ls_out, d_ts_out, h_mtr_out, &done)) || done) return rc;
	const size_t N = pl->N, Tn = h_first[B] - h_first[0], first0 = h_first[0];
	// K of every row (refused before anything is written where one does not fit its count); the ensembles with traces
	std::vector<Ens> E;
	std::vector<unsigned> Kc((size_t)B * M, 0);
	unsigned max_count = 0;
	for (unsigned b = 0; b < B; b++) {
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		for (unsigned q = 0; q < M; q++) {
			const unsigned char *row = h_cnt + (size_t)q * Tn + (f - first0);
			size_t K = 0;
			for (size_t i = 0; i < m; i++) { K += row[i]; max_count = std::max<unsigned>(max_count, row[i]); }
			if (K > 0xffffffffull) return fail(TSPWS_E_ARG, "bootstrap_batch: more than 2^32 copies in one replica");
			Kc[(size_t)b * M + q] = (unsigned)K;
		}
		if (m) E.push_back(Ens{b, f, m});
	}
	memcpy(h_mtr_out, Kc.data(), Kc.size() * sizeof(unsigned));
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_boot_batch_stats &stats = pl->boot_batch_stats;
	stats = tspws_hip_boot_batch_stats();
	stats.shared = (unsigned)E.size();
	stats.empty = B - (unsigned)E.size();
	stats.rows = (unsigned)(E.size() * M);
	stats.max_count = max_count;
	BatchCall call(st);
	// the statistic over the replicas, from the float rows a round has just written (grid.y: a round's ensembles)
	auto moments = [&](const SbEns *d_ens, const unsigned *d_kc, unsigned ne) {
		if (d_stats)
			hipLaunchKernelGGL(k_bt_moments, dim3((unsigned)((N + 255) / 256), ne), dim3(256), 0, st, (const float *)d_ls_out, (const float *)d_ts_out, N, d_ens, d_kc, M, d_stats);
	};
	if (!E.empty() && (rc = row_batch_rounds(pl, p, d_x, ld, first0, E, M, CountRows{h_cnt}, Tn, d_ls_out, d_ts_out, h_mtr_out, stats.rounds, call, moments))) return rc;
	// empty ensembles: zero rows and statistics (their counts are zero already)
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls_out, (size_t)M * N}, {d_ts_out, (size_t)M * N}, {d_stats, 4 * N}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_bootstrap_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                         float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, float *d_stats, void *s)
{
	bool done;
	int rc;
	if ((rc = check_args(pl, p, d_x, ld, h_first, B, M, true, d_ls_out, d_ts_out, h_mtr_out, &done)) || done) return rc;
	// the counts before the first device call: the initialisation of the HIP runtime consumes libc rand() values (see tspws_hip_subsample_sel)
	std::vector<unsigned char> cnt((size_t)M * (h_first[B] - h_first[0]) + 1);
	if (tspws_bootstrap_plan_batch(cnt.data(), h_first, B, M)) return fail(TSPWS_E_ARG, "bootstrap_batch: the draw refused its arguments"); // (cannot happen)
	return tspws_hip_bootstrap_batch_cnt(pl, p, d_x, ld, h_first, B, M, cnt.data(), d_ls_out, d_ts_out, h_mtr_out, d_stats, s);
}

extern "C" int tspws_hip_bootstrap_batch_stats(const tspws_hip_plan *pl, tspws_hip_boot_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "bootstrap_batch_stats: NULL");
	*stats = pl->boot_batch_stats;
	return 0;
}
