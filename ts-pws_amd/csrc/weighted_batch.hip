// weighted_batch.hip -- real-weighted stacks of many ensembles in one call (tspws_hip_weighted_stack_batch).  Reference citations are relative
// to the reference project's src/ directory.
//
// The reference's linear stack takes a weight per trace (tspws_stacks_float, ts_pws1f_lib.c:485-490) that nothing ever passes and that leaves the
// phase stack and the normalisers unweighted.  Row (b, m) here is the consistent form: with w_i >= 0 the weights of row m on the traces of
// ensemble b, n+ the traces with w_i > 0, W = sum w_i, Q = sum w_i^2 and Keff = W W / Q,
//   ST = sum w_i Y_i, PS = sum w_i Y_i / |Y_i|, coherence c = |PS| / W, bias of c^2 for random phases = Q / W^2 = 1 / Keff.
//   host       n+, W, Q, Keff of every row (FP64, trace order)
//   rounds     those of row_batch.h with an FP64 weight as a row's code of a trace (WeightRows): the 8 weights of a trace in one aligned
//              64-byte block, read through a wave-uniform address; a weight adds w times coefficient and phasor -- one fused multiply-add per
//              component -- and a zero weight skips the trace; the linear stack's addend is w x, rounded on its own, its divisor W; the
//              finish is k_wb_weight with each row's (n+, W, Keff)
// A 0/1 row runs exactly the arithmetic of a mask row of sub_batch.hip (fma(1, a, s) = s + a), and W = Keff = K gives weight_value(K, K).
// Two-stage ensembles are refused by design: with real weights the groups floor(k Kmax / K) have no meaning.
#include "tspws_internal.h"
#include "row_batch.h"

// the 8 weights of one trace in the rows 8 g .. 8 g + 7 (rows past M: zero)
struct alignas(64) Wb8 { double w[8]; };
// what the finish needs of a row: W = sum w and Keff = W W / Q (n+ travels as the row's count, the Kc of k_sb_epilogue)
struct WbRow { double W, Keff; };

// a double as a wave-uniform value: that of the first active lane
__device__ __forceinline__ double readfirstlane_f64(const double x)
{
	const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
	return __hiloint2double(hi, lo);
}

// weighted coefficients of the rows r0 + blockIdx.y of the round: OUT = ST * weight(PS; W, Keff), the mode by the row's n+ (n+ = 1: the K = 1
// rule, ts_pws1f_lib.c:972, and so does a row whose Keff is exactly 1); n+ = 0: a zero set
__global__ void __launch_bounds__(256) k_wb_weight(double2 *__restrict__ OUT, const double2 *__restrict__ planes, size_t ncoef, const unsigned *__restrict__ npos,
                                                   const WbRow *__restrict__ rows, size_t r0, double wu, int unbiased)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= ncoef) return;
	const size_t r = r0 + blockIdx.y;
	const unsigned np = npos[r];
	double2 o = make_double2(0, 0);
	// (Keff == 1 with n+ > 1: one weight carries the row in FP64 -- the K = 1 rule as well, Keff - 1 = 0 removes no bias)
	if (np) o = weight_value_eff(planes[r * 2 * ncoef + i], planes[r * 2 * ncoef + ncoef + i], j1_weight_mode(wu, unbiased, rows[r].Keff == 1. ? 1u : np), rows[r].W, rows[r].Keff, rows[r].W, wu);
	OUT[(size_t)blockIdx.y * ncoef + i] = o;
}

// a row's code of a trace: its weight (rows past M: zero)
struct WeightRows {
	using Entry = Wb8;
	using Value = double;
	using Codes = Wb8;
	using Lane = double;
	using Code = double;
	using Row = WbRow;
	struct Rows { // n+ as the count, W as the divisor
		const unsigned *kc;
		const WbRow *rows;
		static Rows at(const unsigned *kc, const void *rows) { return {kc, (const WbRow *)rows}; }
		__device__ double total(size_t r) const { return rows[r].W; }
	};
	static constexpr bool CODES_AHEAD = true, LOAD_ALL = true;
	static constexpr unsigned SPARE = 3; // (k_rb_accumulate loads the blocks of four traces at a time, whatever the ensemble's size)
	static constexpr const char *NAME = "weighted_stack_batch", *ROWS = "rows";
	const Value *h;
	const Row *h_rows;
	static void put(Entry &e, unsigned lane, Value v) { e.w[lane] = v; }
	static void launch_weight(dim3 grid, hipStream_t st, double2 *OUT, const double2 *planes, size_t nc, const Rows &rows, size_t r0, const t_tsPWS *p)
	{
		hipLaunchKernelGGL(k_wb_weight, grid, dim3(256), 0, st, OUT, planes, nc, rows.kc, rows.rows, r0, p->wu, p->unbiased);
	}
	static __device__ __forceinline__ Codes fetch(const Entry *t)
	{
		Codes c;
#pragma unroll
		for (int m = 0; m < 8; m++) c.w[m] = readfirstlane_f64(t->w[m]);
		return c;
	}
	static __device__ __forceinline__ void add(const Codes &c, int m, double2 &st, double2 &ps, const double2 &a, const double2 &u)
	{
		const double w = c.w[m];
		if (w != 0.) { // a trace without weight takes no part: never 0 * Y
			st.x = fma(w, a.x, st.x); st.y = fma(w, a.y, st.y);
			ps.x = fma(w, u.x, ps.x); ps.y = fma(w, u.y, ps.y);
		}
	}
	static __device__ __forceinline__ Code code(Lane x, unsigned) { return x; }
	static __device__ __forceinline__ float add(float acc, Code c, float v)
	{
#pragma clang fp contract(off) // w x is rounded before it is added
		return c != 0. ? (float)((double)acc + c * (double)v) : acc;
	}
};

extern "C" int tspws_hip_weighted_stack_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                              const double *h_w, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, double *h_keff, void *s)
{
	// n+, W, Keff of every row (refused before anything is written, and before the plan is looked at); the ensembles with traces
	std::vector<Ens> E;
	std::vector<unsigned> np;
	std::vector<WbRow> rows;
	auto weights = [&]() {
#pragma clang fp contract(off) // W, Q and Keff: every operation rounded on its own
		const size_t Tn = h_first[B] - h_first[0];
		np.assign((size_t)B * M, 0);
		rows.assign((size_t)B * M, WbRow{0, 0});
		for (unsigned b = 0; b < B; b++) {
			const size_t f = h_first[b], m = h_first[b + 1] - f;
			for (unsigned q = 0; q < M; q++) {
				const double *row = h_w + (size_t)q * Tn + (f - h_first[0]);
				double W = 0, Q = 0;
				unsigned k = 0;
				for (size_t i = 0; i < m; i++) {
					const double w = row[i];
					if (!(w >= 0) || !std::isfinite(w)) return fail(TSPWS_E_ARG, "weighted_stack_batch: a weight that is NaN, infinite or negative");
					W += w; Q += w * w; k += w > 0;
				}
				if (!std::isfinite(W) || !std::isfinite(Q)) return fail(TSPWS_E_ARG, "weighted_stack_batch: the sum of a row's weights or of their squares is not finite");
				if (k && !(Q > 0)) return fail(TSPWS_E_ARG, "weighted_stack_batch: the squares of a row's weights underflow (scale the weights)");
				np[(size_t)b * M + q] = k;
				if (k) rows[(size_t)b * M + q] = WbRow{W, W * W / Q};
			}
			if (m) E.push_back(Ens{b, f, m});
		}
		return 0;
	};
	bool done;
	int rc;
	if ((rc = row_batch_check(WeightRows::NAME, "a two-stage ensemble (0 < Kmax <= its traces): with real weights the groups of the two-stage stack have no meaning, only single-stage ensembles",
	                          pl, p, d_x, ld, h_first, B, M, h_w != nullptr, d_ls_out, d_ts_out, h_mtr_out, &done, weights)) || done) return rc;
	const size_t N = pl->N, Tn = h_first[B] - h_first[0];
	memcpy(h_mtr_out, np.data(), np.size() * sizeof(unsigned));
	if (h_keff) for (size_t r = 0; r < rows.size(); r++) h_keff[r] = rows[r].Keff;
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_weighted_batch_stats &stats = pl->weighted_batch_stats;
	stats = tspws_hip_weighted_batch_stats();
	stats.shared = (unsigned)E.size();
	stats.empty = B - (unsigned)E.size();
	stats.rows = (unsigned)(E.size() * M);
	BatchCall call(st);
	if (!E.empty() && (rc = row_batch_rounds(pl, p, d_x, ld, h_first[0], E, M, WeightRows{h_w, rows.data()}, Tn, d_ls_out, d_ts_out, np.data(), stats.rounds, call,
	                                        [](const SbEns *, const unsigned *, unsigned) {}))) return rc;
	// empty ensembles: zero rows (their counts and Keff are zero already)
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls_out, (size_t)M * N}, {d_ts_out, (size_t)M * N}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_weighted_stack_batch_stats(const tspws_hip_plan *pl, tspws_hip_weighted_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "weighted_stack_batch_stats: NULL");
	*stats = pl->weighted_batch_stats;
	return 0;
}
