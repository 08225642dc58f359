// trace_scores.hip -- which traces belong in the stack: the reference's two figures of merit (similarity, ts_pws1f_lib.c:433-449; misfit,
// :452-462) of every TRACE of B ensembles against R reference rows per ensemble (tspws_hip_trace_scores), and the selective stack built on
// them from the batched calls (tspws_hip_selective_stack_batch: stack, score, select, restack; no kernel of its own).
//
// One pass that reads every trace sample of the lag window once from HBM (16-byte non-temporal loads, the vector / scalar rule of
// stream.hip); the reference rows of an ensemble (at most 4 x 512 KB) come back from L2.  All sums are FP64 with explicit fma: products of
// two floats are exact there, so dot and xx carry summation error only.
//   host       per round ONE table of groups (up to TS_TR consecutive traces of one ensemble) and one upload; rounds of whole ensembles so
//              that the partial sums stay inside TSPWS_PART_MB
//   k_ts_partial<R, VEC>  one WAVE per (group, column segment of TS_W samples): a lane walks its columns of the segment for the group's
//              traces side by side -- the reference samples are loaded and converted once per group, not once per trace -- and keeps xx,
//              and per reference dot, misfit and rr, in registers; then ONE 64-lane reduce-scatter per trace (valu_reduce16, lane_reduce.h)
//              leaves the 1 + 3 R sums of (trace, segment) in 16 lanes, which store them: part[trace][segment][16]
//   k_ts_final one thread per (trace, reference): adds the segments in segment order and forms sim = dot / sqrt(xx) / sqrt(rr)
// Waves never talk to each other (no LDS, no barrier), nothing is atomic, every output has one writer: a repeated call is bit-identical.
// The accumulators of a trace see only that trace and its reference rows, in an order fixed by the window and the route: grouping, batching
// and the other references of the call change no bit.  Window edges that are no multiple of 4 are a scalar head (first segment) and tail
// (last segment) of at most 3 samples each, never a misaligned vector load.  Columns max .. ld-1 are never read.
#include "tspws_internal.h"
#include "batch_host.h"
#include "lane_reduce.h"

enum { TS_W = 4096, TS_TR = 4, TS_NV = 16, TS_RMAX = 4 }; // samples per column segment, traces per group, doubles per (trace, segment) slot

// up to TS_TR consecutive traces of ensemble b: t0 = the first one's row in d_sigall
struct TsGroup { unsigned long long t0; unsigned count, b; };

// the lag window [n0, n1) and its aligned body [a0, a1) (vector route; a0 >= a1: no body), nseg column segments
struct TsWin { unsigned long long n0, n1, a0, a1; unsigned nseg; };

typedef float ts_v4f __attribute__((ext_vector_type(4)));

// part[(trace - tbase) nseg + seg][e]: e = 0 xx, 1 + 3k dot_k, 2 + 3k misfit_k, 3 + 3k rr_k
template <int R, bool VEC>
__global__ void __launch_bounds__(256) k_ts_partial(const float *__restrict__ x, size_t ld, const float *__restrict__ ref, size_t ldr, const TsGroup *__restrict__ groups,
                                                    unsigned long long nitems, const TsWin w, unsigned long long tbase, double *__restrict__ part)
{
#pragma clang fp contract(off) // x - r is rounded before it is squared; the sums are explicit fma
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long item = (unsigned long long)blockIdx.x * 4 + wave;
	if (item >= nitems) return; // (the whole wave)
	const unsigned long long g = item / w.nseg;
	const unsigned seg = (unsigned)(item - g * w.nseg);
	const TsGroup gr = groups[g];
	const unsigned count = (unsigned)__builtin_amdgcn_readfirstlane((int)gr.count);
	const float *xp[TS_TR], *rp[R];
#pragma unroll
	for (int j = 0; j < TS_TR; j++) xp[j] = x + (gr.t0 + ((unsigned)j < count ? (unsigned)j : count - 1)) * ld; // (rows past the group: its last row again, not stored)
#pragma unroll
	for (int k = 0; k < R; k++) rp[k] = ref + ((size_t)gr.b * R + k) * ldr;

	double xx[TS_TR], dot[TS_TR][R], mis[TS_TR][R], rr[R];
#pragma unroll
	for (int j = 0; j < TS_TR; j++) {
		xx[j] = 0;
#pragma unroll
		for (int k = 0; k < R; k++) { dot[j][k] = 0; mis[j][k] = 0; }
	}
#pragma unroll
	for (int k = 0; k < R; k++) rr[k] = 0;
	// one column of the group: the reference samples once, then every trace
	auto column = [&](const float (&xv)[TS_TR], const float (&rv)[R]) {
		double rd[R];
#pragma unroll
		for (int k = 0; k < R; k++) { rd[k] = (double)rv[k]; rr[k] = fma(rd[k], rd[k], rr[k]); }
#pragma unroll
		for (int j = 0; j < TS_TR; j++) {
			const double xd = (double)xv[j];
			xx[j] = fma(xd, xd, xx[j]);
#pragma unroll
			for (int k = 0; k < R; k++) {
				dot[j][k] = fma(xd, rd[k], dot[j][k]);
				const double d = xd - rd[k];
				mis[j][k] = fma(d, d, mis[j][k]);
			}
		}
	};
	auto scalar_column = [&](const unsigned long long c) {
		float xv[TS_TR], rv[R];
#pragma unroll
		for (int j = 0; j < TS_TR; j++) xv[j] = xp[j][c];
#pragma unroll
		for (int k = 0; k < R; k++) rv[k] = rp[k][c];
		column(xv, rv);
	};

	if (VEC) {
		// head of the window in front of the aligned body (first segment), at most 3 samples: one lane each
		const unsigned long long hend = w.a0 < w.n1 ? w.a0 : w.n1;
		if (seg == 0 && w.n0 + lane < hend) scalar_column(w.n0 + lane);
		if (w.a0 < w.a1) {
			const unsigned long long lo = w.a0 + (unsigned long long)seg * TS_W, hi = lo + TS_W < w.a1 ? lo + TS_W : w.a1;
			auto vec_column = [&](const unsigned long long c) {
				ts_v4f xq[TS_TR], rq[R];
#pragma unroll
				for (int j = 0; j < TS_TR; j++) xq[j] = __builtin_nontemporal_load((const ts_v4f *)(xp[j] + c));
#pragma unroll
				for (int k = 0; k < R; k++) rq[k] = *(const ts_v4f *)(rp[k] + c);
#pragma unroll
				for (int q = 0; q < 4; q++) {
					float xv[TS_TR], rv[R];
#pragma unroll
					for (int j = 0; j < TS_TR; j++) xv[j] = xq[j][q];
#pragma unroll
					for (int k = 0; k < R; k++) rv[k] = rq[k][q];
					column(xv, rv);
				}
			};
			const unsigned nfull = (unsigned)((hi - lo) / 256); // whole steps of the wave: 64 lanes x 4 samples
			unsigned long long c = lo + (unsigned long long)lane * 4;
#pragma unroll 2
			for (unsigned it = 0; it < nfull; it++, c += 256) vec_column(c);
			if (c < hi) vec_column(c); // (hi - lo is a multiple of 4: a lane's four samples are inside or outside together)
		}
		// tail behind the aligned body (last segment)
		if (seg == w.nseg - 1 && w.a0 < w.n1 && w.a1 + lane < w.n1) scalar_column(w.a1 + lane);
	} else {
		const unsigned long long lo = w.n0 + (unsigned long long)seg * TS_W, hi = lo + TS_W < w.n1 ? lo + TS_W : w.n1;
		for (unsigned long long c = lo + lane; c < hi; c += 64) scalar_column(c);
	}

	// every lane is back here: one reduce-scatter per trace, 16 lanes store the slot
	const unsigned e = ((lane >> 5) & 1u) * 8 + ((lane >> 4) & 1u) * 4 + ((lane >> 3) & 1u) * 2 + ((lane >> 2) & 1u);
#pragma unroll
	for (int j = 0; j < TS_TR; j++) {
		if ((unsigned)j >= count) break; // (wave-uniform)
		double v[TS_NV];
#pragma unroll
		for (int i = 0; i < TS_NV; i++) v[i] = 0;
		v[0] = xx[j];
#pragma unroll
		for (int k = 0; k < R; k++) { v[1 + 3 * k] = dot[j][k]; v[2 + 3 * k] = mis[j][k]; v[3 + 3 * k] = rr[k]; }
		const double r = valu_reduce16(v, lane);
		if ((lane & 3u) == 0) part[((gr.t0 + (unsigned)j - tbase) * w.nseg + seg) * TS_NV + e] = r;
	}
}

// scores[k][sim | misfit | dot][col0 + t] and energy[col0 + t] of the nt traces of a round: the segments' sums in segment order
__global__ void __launch_bounds__(256) k_ts_final(const double *__restrict__ part, unsigned nseg, unsigned long long nt, unsigned R, unsigned long long col0,
                                                  unsigned long long T, double *__restrict__ scores, double *__restrict__ energy)
{
#pragma clang fp contract(off)
	const unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (idx >= nt * R) return;
	const unsigned k = (unsigned)(idx / nt);
	const unsigned long long t = idx - (unsigned long long)k * nt;
	const double *p = part + t * nseg * TS_NV;
	double xx = 0, dot = 0, mis = 0, rr = 0;
	for (unsigned s = 0; s < nseg; s++, p += TS_NV) { xx += p[0]; dot += p[1 + 3 * k]; mis += p[2 + 3 * k]; rr += p[3 + 3 * k]; }
	double *o = scores + (size_t)k * 3 * T + col0 + t;
	o[0] = dot / sqrt(xx) / sqrt(rr); // (the reference's similarity with the trace as x1: 0 / 0 = NaN for a dead trace or reference)
	o[T] = mis;
	o[2 * T] = dot;
	if (energy && k == 0) energy[col0 + t] = xx;
}

namespace {

template <int R>
void launch_partial(bool vec, unsigned long long nitems, hipStream_t st, const float *x, size_t ld, const float *ref, size_t ldr, const TsGroup *groups, const TsWin &w,
                    unsigned long long tbase, double *part)
{
	const dim3 grid((unsigned)((nitems + 3) / 4));
	if (vec) hipLaunchKernelGGL((k_ts_partial<R, true>), grid, dim3(256), 0, st, x, ld, ref, ldr, groups, nitems, w, tbase, part);
	else hipLaunchKernelGGL((k_ts_partial<R, false>), grid, dim3(256), 0, st, x, ld, ref, ldr, groups, nitems, w, tbase, part);
}

// what the scores and the selective stack both refuse about the window, once the plan's trace length is known; n1 == 0 becomes max
const char *window_of(size_t N, size_t n0, size_t &n1)
{
	if (!n1) n1 = N;
	if (n0 >= n1) return "an empty lag window (n0 >= n1)";
	if (n1 > N) return "a lag window past the trace length";
	return nullptr;
}

} // namespace

extern "C" int tspws_hip_trace_scores(tspws_hip_plan *pl, const float *d_x, size_t ld, const size_t *h_first, unsigned B, const float *d_ref, size_t ldr, unsigned R,
                                      size_t n0, size_t n1, double *d_scores, double *d_energy, void *s)
{
	// first what needs no plan
	if (!h_first) return fail(TSPWS_E_ARG, "trace_scores: NULL");
	if (!R || R > TS_RMAX) return fail(TSPWS_E_ARG, "trace_scores: 1 to 4 reference rows per ensemble");
	if (n1 && n0 >= n1) return fail(TSPWS_E_ARG, "trace_scores: an empty lag window (n0 >= n1)");
	if (!B) return pl ? 0 : fail(TSPWS_E_ARG, "trace_scores: NULL");
	if (!d_ref || !d_scores) return fail(TSPWS_E_ARG, "trace_scores: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "trace_scores: decreasing ensemble offsets");
	if (!pl) return fail(TSPWS_E_ARG, "trace_scores: NULL");
	const size_t N = pl->N, T = h_first[B] - h_first[0], first0 = h_first[0];
	if (T && !d_x) return fail(TSPWS_E_ARG, "trace_scores: NULL traces");
	if (ld < N) return fail(TSPWS_E_ARG, "trace_scores: row stride below the trace length");
	if (ldr < N) return fail(TSPWS_E_ARG, "trace_scores: reference row stride below the trace length");
	if (const char *bad = window_of(N, n0, n1)) return fail(TSPWS_E_ARG, (std::string("trace_scores: ") + bad).c_str());
	if (!T) return 0;

	// the route: stream.hip's rule for the traces, the same for the references
	const bool vec = N % 4 == 0 && ld % 4 == 0 && ((uintptr_t)d_x & 15) == 0 && ldr % 4 == 0 && ((uintptr_t)d_ref & 15) == 0;
	TsWin w;
	w.n0 = n0; w.n1 = n1;
	w.a0 = (n0 + 3) & ~(size_t)3; w.a1 = n1 & ~(size_t)3;
	const size_t span = vec ? (w.a0 < w.a1 ? w.a1 - w.a0 : 0) : n1 - n0;
	w.nseg = (unsigned)std::max<size_t>(1, (span + TS_W - 1) / TS_W);
	const size_t slot = (size_t)w.nseg * TS_NV * sizeof(double), budget = tspws_part_budget_bytes();

	// rounds of whole ensembles: the partial sums of a round and its group table within the budget
	std::vector<size_t> g0((size_t)B + 1, 0); // groups in front of ensemble b
	for (unsigned b = 0; b < B; b++) g0[b + 1] = g0[b] + (h_first[b + 1] - h_first[b] + TS_TR - 1) / TS_TR;
	auto bytes_of = [&](size_t j0, size_t j1) { return (h_first[j1] - h_first[j0]) * slot + (g0[j1] - g0[j0]) * sizeof(TsGroup); };
	const std::vector<Round> rounds = whole_ensemble_rounds(B, [&](size_t j0, size_t j1) { return bytes_of(j0, j1) <= budget; });
	size_t max_part = 0, max_tab = 0;
	for (const Round &r : rounds) {
		if (((g0[r.j1] - g0[r.j0]) * w.nseg + 3) / 4 > 0x7fffffffull) // (one workgroup per 4 waves: the launch's grid)
			return fail(TSPWS_E_ARG, "trace_scores: more than 2^33 (group, segment) waves in a round");
		max_part = std::max(max_part, (h_first[r.j1] - h_first[r.j0]) * slot);
		max_tab = std::max(max_tab, (g0[r.j1] - g0[r.j0]) * sizeof(TsGroup));
	}

	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_trace_scores_stats_t &stats = pl->trace_scores_stats;
	stats = tspws_hip_trace_scores_stats_t();
	stats.vec = vec; stats.segments = w.nseg;
	for (unsigned b = 0; b < B; b++) stats.empty += h_first[b + 1] == h_first[b];
	BatchCall call(st);
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_TSP, std::max<size_t>(max_part, 16), &v))) return rc; // (the largest round's: the slot does not grow between rounds)
	double *part = (double *)v;
	for (const Round &r : rounds) {
		const size_t nt = h_first[r.j1] - h_first[r.j0], ng = g0[r.j1] - g0[r.j0];
		if (!nt) continue; // (a round of empty ensembles)
		stats.rounds++;
		char *blob = call.block(ng * sizeof(TsGroup)), *tab;
		TsGroup *hg = (TsGroup *)blob;
		for (size_t b = r.j0; b < r.j1; b++)
			for (size_t t = h_first[b]; t < h_first[b + 1]; t += TS_TR) {
				TsGroup d;
				d.t0 = t; d.count = (unsigned)std::min<size_t>(TS_TR, h_first[b + 1] - t); d.b = (unsigned)b;
				*hg++ = d;
			}
		if ((rc = call.upload(pl, SCR_TSTAB, blob, ng * sizeof(TsGroup), &tab, max_tab))) return rc;
		const unsigned long long nitems = (unsigned long long)ng * w.nseg;
		const TsGroup *d_groups = (const TsGroup *)tab;
		switch (R) {
		case 1: launch_partial<1>(vec, nitems, st, d_x, ld, d_ref, ldr, d_groups, w, h_first[r.j0], part); break;
		case 2: launch_partial<2>(vec, nitems, st, d_x, ld, d_ref, ldr, d_groups, w, h_first[r.j0], part); break;
		case 3: launch_partial<3>(vec, nitems, st, d_x, ld, d_ref, ldr, d_groups, w, h_first[r.j0], part); break;
		default: launch_partial<4>(vec, nitems, st, d_x, ld, d_ref, ldr, d_groups, w, h_first[r.j0], part); break;
		}
		hipLaunchKernelGGL(k_ts_final, dim3((unsigned)((nt * R + 255) / 256)), dim3(256), 0, st, (const double *)part, w.nseg, (unsigned long long)nt, R,
		                   (unsigned long long)(h_first[r.j0] - first0), (unsigned long long)T, d_scores, d_energy);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // scores complete
	return 0;
}

extern "C" int tspws_hip_trace_scores_stats(const tspws_hip_plan *pl, tspws_hip_trace_scores_stats_t *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "trace_scores_stats: NULL");
	*stats = pl->trace_scores_stats;
	return 0;
}

extern "C" int tspws_hip_selective_stack_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, int against,
                                               int rule, double a, unsigned iters, size_t n0, size_t n1, float *d_ls, float *d_ts, char *h_sel, unsigned *h_kept,
                                               unsigned *iters_done, void *s)
{
	// first what needs no plan, in the order of the composed calls
	if (!p || !h_first) return fail(TSPWS_E_ARG, "selective_stack_batch: NULL");
	if (against != 0 && against != 1) return fail(TSPWS_E_ARG, "selective_stack_batch: against is 0 (ls) or 1 (tsPWS)");
	if ((rule != 0 && rule != 1) || a != a) return fail(TSPWS_E_ARG, "selective_stack_batch: an unknown rule or a NaN threshold");
	if (!iters) return fail(TSPWS_E_ARG, "selective_stack_batch: iters == 0");
	if (n1 && n0 >= n1) return fail(TSPWS_E_ARG, "selective_stack_batch: an empty lag window (n0 >= n1)");
	if (!B) return pl ? 0 : fail(TSPWS_E_ARG, "selective_stack_batch: NULL");
	if (!d_ls || !d_ts || !h_sel || !h_kept) return fail(TSPWS_E_ARG, "selective_stack_batch: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "selective_stack_batch: decreasing ensemble offsets");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] - h_first[b] > 0xfffffff0ull) return fail(TSPWS_E_ARG, "selective_stack_batch: more than 2^32 traces in an ensemble");
	if (!pl) return fail(TSPWS_E_ARG, "selective_stack_batch: NULL");
	const size_t N = pl->N, T = h_first[B] - h_first[0];
	if (T && !d_x) return fail(TSPWS_E_ARG, "selective_stack_batch: NULL traces");
	if (ld < N) return fail(TSPWS_E_ARG, "selective_stack_batch: row stride below the trace length");
	if (const char *bad = window_of(N, n0, n1)) return fail(TSPWS_E_ARG, (std::string("selective_stack_batch: ") + bad).c_str());

	HIP_TRY(hipSetDevice(pl->device));
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_TSOUT, std::max<size_t>(3 * T * sizeof(double), 16), &v))) return rc;
	double *d_scores = (double *)v;
	std::vector<double> sim(T);
	std::vector<char> next(T);
	unsigned done = 0;
	// pass 0 scores against the plain stacks, every further pass against the rows the previous pass wrote; each of the composed calls waits for the stream
	if ((rc = tspws_hip_stack_batch(pl, p, d_x, ld, h_first, B, d_ls, d_ts, s))) return rc;
	for (unsigned pass = 0; pass < iters; pass++) {
		if ((rc = tspws_hip_trace_scores(pl, d_x, ld, h_first, B, against ? d_ts : d_ls, N, 1, n0, n1, d_scores, nullptr, s))) return rc;
		if (T) HIP_TRY(hipMemcpy(sim.data(), d_scores, T * sizeof(double), hipMemcpyDeviceToHost)); // (the sim plane; the stream is drained)
		if (tspws_selection_from_scores(next.data(), nullptr, sim.data(), h_first, B, rule, a)) return fail(TSPWS_E_ARG, "selective_stack_batch: selection refused");
		if (pass && !memcmp(next.data(), h_sel, T)) break; // the mask stands: the rows are those of this mask already
		if (T) memcpy(h_sel, next.data(), T);
		if ((rc = tspws_hip_subsample_batch_sel(pl, p, d_x, ld, h_first, B, 1, h_sel, d_ls, d_ts, h_kept, s))) return rc;
		done++;
	}
	if (iters_done) *iters_done = done;
	return 0;
}
