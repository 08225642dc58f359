// sub_batch.hip -- random subsamples of many ensembles in one call (tspws_hip_subsample_batch, tspws_hip_subsample_batch_sel), the host draw of
// their masks and the selections / weights from trace scores.  Reference citations are relative to the reference project's src/ directory.
//
// tspws_hip_subsample_sel gives the M random subsamples of ONE ensemble: per call a mask upload, a memset, a forward launch over a few dozen
// traces, k_accumulate_masked, k_sub_linear, a weight launch, an inverse over M rows, an epilogue and a wait.  The batched jackknives cannot
// stand in: under random masks nearly every trace is a selection class of its own (jk_batch.hip pads every class to a 64-trace block), and
// the single-stage subsampling body forms its linear rows with a FLOAT accumulator (ts_pws1f_lib.c:538-542).  This unit does the batch at once;
// every ensemble follows the single call's rule on its own size (two-stage iff 0 < Kmax <= M_b), and a batch may mix both kinds.
//   host       K_{b,m} of every (ensemble, mask); the ensembles with traces in two lists, single-stage and two-stage
//   single     the rounds of row_batch.h with a mask bit as a row's code of a trace (MaskRows): the 8 mask bits of a trace in one byte, a
//              set bit adds the trace once
//   two-stage  the shared walk of jk_batch_two_stage.hip over that list, without main rows (tspws_jb2_shared; its own rounds)
// A batch with ONE non-empty ensemble is tspws_hip_subsample_sel for it (a single-stage one: when every row has the K that call derives
// from subsmpl_p).
#include "tspws_internal.h"
#include "row_batch.h"

#define is_two_stage tspws_is_two_stage

// a row's code of a trace: one mask bit (bits past M are zero)
struct MaskRows {
	using Entry = unsigned char;
	using Value = char;
	using Codes = unsigned;
	using Lane = unsigned char;
	using Code = bool;
	using Rows = KRows;
	using Row = void;
	static constexpr bool CODES_AHEAD = false, LOAD_ALL = false; // (a dropped trace is not loaded)
	static constexpr unsigned SPARE = 0;
	static constexpr const char *NAME = "subsample_batch", *ROWS = "mask rows";
	static constexpr auto launch_weight = launch_sb_weight;
	const Value *h;
	static void put(Entry &e, unsigned lane, Value v) { if (v == 1) e |= (Entry)(1u << lane); }
	static __device__ __forceinline__ Codes fetch(const Entry *t) { return (unsigned)__builtin_amdgcn_readfirstlane((int)*t); }
	static __device__ __forceinline__ void add(Codes mb, int m, double2 &st, double2 &ps, const double2 &a, const double2 &u)
	{
		if ((mb >> m) & 1u) { st.x += a.x; st.y += a.y; ps.x += u.x; ps.y += u.y; } // (wave-uniform)
	}
	static __device__ __forceinline__ Code code(Lane x, unsigned lane) { return (x >> lane) & 1u; }
	static __device__ __forceinline__ float add(float acc, Code c, float v) { return c ? (float)((double)acc + (double)v) : acc; }
};

namespace {

// what both entries refuse (row_batch_check; two-stage ensembles are taken)
int check_args(const tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M, bool sel_ok,
               const float *d_ls_out, const float *d_ts_out, const unsigned *h_mtr_out, bool *done)
{
	return row_batch_check(MaskRows::NAME, nullptr, pl, p, d_x, ld, h_first, B, M, sel_ok, d_ls_out, d_ts_out, h_mtr_out, done, [] { return 0; });
}

} // namespace

extern "C" int tspws_subsampling_plan_batch(char *sel, const size_t *first, unsigned B, unsigned M, double prob)
{
	if (!sel || !first) return 1;
	for (unsigned b = 0; b < B; b++) if (first[b + 1] < first[b]) return 1;
	const size_t T = first[B] - first[0];
	for (unsigned b = 0; b < B; b++) {
		const size_t m = first[b + 1] - first[b];
		if (!m) continue;
		const size_t K = (size_t)ceil((double)m * prob); // (tspws_hip_subsample's K)
		for (unsigned q = 0; q < M; q++)
			if (int rc = tspws_subsampling_plan(sel + (size_t)q * T + (first[b] - first[0]), m, K)) return rc;
	}
	return 0;
}

// median of v[0 .. n) (n > 0; sorted in place): for an even count 0.5 * (lo + hi) of the two middle order statistics
static double median_inplace(double *v, size_t n)
{
	std::sort(v, v + n);
	return n & 1 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

extern "C" int tspws_selection_from_scores(char *sel, unsigned *kept, const double *score, const size_t *first, unsigned B, int rule, double a)
{
#pragma clang fp contract(off) // med - a * 1.4826 * mad, every operation rounded on its own
	if (!sel || !score || !first) return 1;
	for (unsigned b = 0; b < B; b++) if (first[b + 1] < first[b]) return 1;
	if ((rule != 0 && rule != 1) || a != a) return 2;
	std::vector<double> v;
	for (unsigned b = 0; b < B; b++) {
		const size_t c0 = first[b] - first[0], m = first[b + 1] - first[b];
		double thr = a;
		bool any = true;
		if (rule == 1) { // robust: median and scaled median absolute deviation of the ensemble's finite scores
			v.clear();
			for (size_t i = 0; i < m; i++) if (std::isfinite(score[c0 + i])) v.push_back(score[c0 + i]);
			any = !v.empty();
			if (any) {
				const double med = median_inplace(v.data(), v.size());
				for (double &x : v) x = fabs(x - med);
				const double mad = median_inplace(v.data(), v.size());
				thr = med - a * 1.4826 * mad;
			}
		}
		unsigned k = 0;
		for (size_t i = 0; i < m; i++) { // (NaN fails every >=)
			const char keep = any && score[c0 + i] >= thr ? 1 : 0;
			sel[c0 + i] = keep;
			k += keep;
		}
		if (kept) kept[b] = k;
	}
	return 0;
}

extern "C" int tspws_hip_subsample_batch_sel(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                             const char *h_sel, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *s)
{
	bool done;
	int rc;
	if ((rc = check_args(pl, p, d_x, ld, h_first, B, M, h_sel != nullptr, d_ls_out, d_ts_out, h_mtr_out, &done)) || done) return rc;
	const size_t N = pl->N, Tn = h_first[B] - h_first[0], first0 = h_first[0];
	// K of every row; the ensembles with traces by kind
	std::vector<Ens> single;
	std::vector<unsigned> two;
	for (unsigned b = 0; b < B; b++) {
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		for (unsigned q = 0; q < M; q++) h_mtr_out[(size_t)b * M + q] = kept_count(h_sel + (size_t)q * Tn + (f - first0), m);
		if (!m) continue;
		if (is_two_stage(p, m)) two.push_back(b);
		else single.push_back(Ens{b, f, m});
	}
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_sub_batch_stats &stats = pl->sub_batch_stats;
	stats = tspws_hip_sub_batch_stats();
	const size_t nonempty = single.size() + two.size();
	stats.empty = B - (unsigned)nonempty;
	stats.rows = (unsigned)(nonempty * M);
	BatchCall call(st);
	// one ensemble: the single call with its columns -- which divides by a row's K = 0 and derives the K of a single-stage ensemble from
	// subsmpl_p, so only without empty rows and, single-stage, with those K
	bool loop = nonempty == 1;
	const unsigned b = !loop ? 0 : two.empty() ? single[0].b : two[0];
	if (loop) {
		const size_t K = (size_t)ceil((double)(h_first[b + 1] - h_first[b]) * p->subsmpl_p);
		for (unsigned q = 0; q < M; q++) loop &= h_mtr_out[(size_t)b * M + q] != 0 && (!two.empty() || h_mtr_out[(size_t)b * M + q] == K);
	}
	if (loop) {
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		const char *sel = ensemble_selection(call, h_sel, M, Tn, f - first0, m);
		stats.looped = 1;
		if ((rc = tspws_hip_subsample_sel(pl, p, d_x + f * ld, ld, m, M, sel, d_ls_out + (size_t)b * M * N, d_ts_out + (size_t)b * M * N, s))) return rc;
	} else {
		if (!single.empty()) {
			stats.single_shared = (unsigned)single.size();
			if ((rc = row_batch_rounds(pl, p, d_x, ld, first0, single, M, MaskRows{h_sel}, Tn, d_ls_out, d_ts_out, h_mtr_out, stats.rounds, call,
			                           [](const SbEns *, const unsigned *, unsigned) {}))) return rc;
		}
		if (!two.empty()) {
			stats.two_stage_shared = (unsigned)two.size();
			// (row_batch_rounds has enqueued every round and kept no pointer: the walk may size the shared slots -- tables, sets, reconstructions -- anew)
			tspws_hip_jk_batch2_stats walk = tspws_hip_jk_batch2_stats();
			if ((rc = tspws_jb2_shared(pl, p, d_x, ld, h_first, two.data(), two.size(), h_sel, Tn, M, false, nullptr, nullptr, d_ls_out, d_ts_out, h_mtr_out, call,
			                           &walk))) return rc;
			stats.rounds += walk.rounds;
		}
	}
	// empty ensembles: zero rows (their counts are zero already)
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls_out, (size_t)M * N}, {d_ts_out, (size_t)M * N}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_subsample_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                         float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *s)
{
	bool done;
	int rc;
	if ((rc = check_args(pl, p, d_x, ld, h_first, B, M, true, d_ls_out, d_ts_out, h_mtr_out, &done)) || done) return rc;
	// the masks before the first device call: the initialisation of the HIP runtime consumes libc rand() values (see tspws_hip_subsample_sel)
	std::vector<char> sel((size_t)M * (h_first[B] - h_first[0]) + 1);
	if (tspws_subsampling_plan_batch(sel.data(), h_first, B, M, p->subsmpl_p)) return fail(TSPWS_E_ARG, "subsample_batch: subsmpl_p outside [0, 1]");
	return tspws_hip_subsample_batch_sel(pl, p, d_x, ld, h_first, B, M, sel.data(), d_ls_out, d_ts_out, h_mtr_out, s);
}

extern "C" int tspws_hip_subsample_batch_stats(const tspws_hip_plan *pl, tspws_hip_sub_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "subsample_batch_stats: NULL");
	*stats = pl->sub_batch_stats;
	return 0;
}

extern "C" int tspws_weights_from_scores(double *w, const double *score, const size_t *first, unsigned B, int rule, double a)
{
	if (!w || !score || !first) return 1;
	for (unsigned b = 0; b < B; b++) if (first[b + 1] < first[b]) return 1;
	if ((rule != 0 && rule != 1) || (rule == 0 && a != a)) return 2;
	for (unsigned b = 0; b < B; b++) {
		const size_t c0 = first[b] - first[0], m = first[b + 1] - first[b];
		if (rule == 0) { // a power of a similarity (NaN fails the >)
			for (size_t i = 0; i < m; i++) w[c0 + i] = score[c0 + i] > 0 ? pow(score[c0 + i], a) : 0.;
			continue;
		}
		// inverse energy, the ensemble's largest weight = 1
		double top = 0;
		for (size_t i = 0; i < m; i++) {
			const double s = score[c0 + i];
			w[c0 + i] = s > 0 && std::isfinite(s) ? 1. / s : 0.;
			top = std::max(top, w[c0 + i]);
		}
		if (top > 0) for (size_t i = 0; i < m; i++) w[c0 + i] /= top;
	}
	return 0;
}
