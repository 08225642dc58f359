// conv_batch.hip -- the convergence curves of many ensembles in one call (tspws_hip_convergence_batch).
// Reference citations are relative to the reference project's src/ directory.
//
// tspws_hip_convergence (resample.hip) gives the curves of ONE ensemble (ts_pws1f_lib.c:247-314): for a 30-trace ensemble a forward launch
// over <= 30 traces, a prefix accumulation, an inverse of 30 rows, a one-workgroup sum per row, five tiny launches per two-stage step and
// three copies to the host.  This unit does B ensembles of one trace array at once:
//   incremental steps   (Tr <= Kmax, or every step without a two-stage rule): the traces of ALL ensembles that take part form one list
//                       (gathered when Kmax cuts the ensembles short, the trace array itself otherwise) and go through the forward kernels in
//                       rounds that do not respect ensemble borders.  k_cb_prefix walks a round's per-trace partials in trace order per
//                       coefficient (the layout and block geometry of k_accumulate_parts), restarts ST / PS where the step table says an
//                       ensemble begins, and writes the weighted coefficient after every trace with that ensemble's running count.  The walk is
//                       cut into chains of whole ensembles (grid.y) so that short ensembles fill the GPU; the chain that begins inside an
//                       ensemble -- the first of a round -- takes the running pair the last round left in a plane pair of the scratch.
//   two-stage steps     (Tr > Kmax), recomputed from scratch like the reference (:266-268): k_cb_step_rows sums the Kmax contiguous groups of
//                       every step of a round in trace order, a workgroup per (step, 256 samples) -- the steps of an ensemble sit side by side in
//                       the launch, so its traces are re-read from L2 --, then ONE forward launch over all rows, ONE accumulation that weights
//                       every stack with its own Tr (WeightArgs::Mv), one batched inverse.
//   metrics             k_cb_dot4: the four sums of a reconstruction against the reference row of ITS ensemble (+ the float cast of the step);
//                       k_cb_linear / k_cb_lin_reduce: the running linear stack with grid.y = ensemble; k_cb_refsq: sum ref_ls^2 per ensemble.
//                       One copy to the host per curve.
// Every sum has a fixed order, nothing is atomic, every output element has one writer.  Rounds keep every block that grows with the traces --
// gathered traces, partials, weighted sets, reconstructions, the inverse's octave buffer, step rows, plane pairs, linear partial sums -- within
// the parts budget (TSPWS_PART_MB); a round of incremental steps may split an ensemble, the two-stage steps are independent, a round of the
// linear curve holds whole ensembles (one alone may exceed the budget).  A batch with ONE non-empty ensemble is tspws_hip_convergence for it.
#include "tspws_internal.h"
#include "batch_host.h"

namespace {

struct CbStep {   // one step of a curve
	unsigned cnt; // traces of its ensemble up to and including it (1: the ensemble begins here)
	unsigned ens; // ensemble: row of the references
	unsigned dst; // entry of the curves / row of the step arrays: trace index - h_first[0]
	unsigned pad;
};

struct CbEns {    // one ensemble of a round of the linear curve
	unsigned long long t0; // first trace (row of the trace array)
	unsigned m, b;         // traces, ensemble index
	unsigned dst, off;     // first entry of the curves, first entry inside the round
};

constexpr unsigned CB_CHAIN = 16; // a chain of the prefix walk: whole ensembles until it has this many steps

} // namespace

// rows of the trace array named by the step table, side by side: out[r] = x[first0 + steps[r].dst]
__global__ void __launch_bounds__(256) k_cb_gather(const float *__restrict__ x, size_t ld, size_t N, size_t first0, const CbStep *__restrict__ steps,
                                                   float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	out[(size_t)blockIdx.y * N + n] = x[(first0 + steps[blockIdx.y].dst) * ld + n];
}

// Segmented prefix accumulation: chain blockIdx.y = the steps [chain[y], chain[y + 1]) of the list, whose transformed traces are `part`
// (step s0 first, npart apart, layout of the scale table sc: what k_accumulate_parts reads, with its block geometry -- blockIdx.x works on one
// scale; scales without splits a thread per coefficient, split scales a wave per coefficient).  ST += Y, PS += Y / |Y| in step order, both
// restarted where steps[s].cnt == 1; after every step the weighted coefficient with K = M = cnt goes to OUT[(s - s0) ncoef + i].  The first chain
// continues the pair in cin ([ST | PS], ncoef each) when it begins inside an ensemble, the last chain leaves its pair in cout (another block: the
// two chains run side by side).
__global__ void __launch_bounds__(256) k_cb_prefix(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                   const CbStep *__restrict__ steps, const unsigned *__restrict__ chain, unsigned s0,
                                                   double2 *__restrict__ OUT, size_t ncoef, const double2 *__restrict__ cin, double2 *__restrict__ cout,
                                                   int mode, int mode1, double wu)
{
	const double2 *cinPS = cin + ncoef;
	double2 *coutPS = cout + ncoef;
	const unsigned bx = blockIdx.x;
	const unsigned t0 = chain[blockIdx.y], t1 = chain[blockIdx.y + 1], ntr = t1 - t0;
	const bool carry_in = blockIdx.y == 0 && steps[t0].cnt != 1, carry_out = blockIdx.y == gridDim.y - 1;
	part += (size_t)(t0 - s0) * npart;
	OUT += (size_t)(t0 - s0) * ncoef;
	steps += t0;
	const unsigned lo = find_block_scale(sc, S, bx, true);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	if (nsplit > 1) {
		// up to 32 partials per coefficient: the lanes of a wave are (8 traces) x (8 lanes that share the partials of a trace); the traces of a
		// round of 8 are then added in step order from their groups' lanes (the arithmetic of k_accumulate_parts' few-trace branch)
		const unsigned k = (bx - sc[lo].acc2_off) * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
		if (k >= Ns) return;
		const unsigned sub = lane & 7, bt = lane >> 3;
		const size_t i = sc[lo].coef_off + k;
		const double2 *p0 = part + sc[lo].part_off + k;
		double2 st = make_double2(0, 0), ps = make_double2(0, 0);
		if (carry_in) { st = cin[i]; ps = cinPS[i]; }
		for (unsigned b0 = 0; b0 < ntr; b0 += 8) {
			const bool on = b0 + bt < ntr;
			const double2 *p = p0 + (size_t)(on ? b0 + bt : 0u) * npart;
			double2 v = make_double2(0.0, 0.0);
			for (unsigned sp = sub; sp < nsplit; sp += 32) {
				double2 t[4];
#pragma unroll
				for (int j = 0; j < 4; j++) t[j] = (on && sp + (unsigned)j * 8u < nsplit) ? p[(size_t)(sp + (unsigned)j * 8u) * Ns] : make_double2(0.0, 0.0);
#pragma unroll
				for (int j = 0; j < 4; j++) { v.x += t[j].x; v.y += t[j].y; }
			}
#pragma unroll
			for (int o = 1; o < 8; o <<= 1) { v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64); }
			const unsigned nb = ntr - b0 < 8u ? ntr - b0 : 8u;
#pragma unroll
			for (int j = 0; j < 8; j++) {
				if ((unsigned)j < nb) {
					const double2 vj = make_double2(readlane_f64(v.x, 8 * j), readlane_f64(v.y, 8 * j));
					const unsigned cnt = steps[b0 + (unsigned)j].cnt;
					if (cnt == 1) { st = make_double2(0, 0); ps = make_double2(0, 0); }
					st.x += vj.x; st.y += vj.y;
					add_unit_phasor(ps, vj);
					if (lane == 0) OUT[(size_t)(b0 + (unsigned)j) * ncoef + i] = weight_value(st, ps, cnt == 1 ? mode1 : mode, (double)cnt, (double)cnt, wu);
				}
			}
		}
		if (carry_out && lane == 0) { cout[i] = st; coutPS[i] = ps; }
		return;
	}
	const unsigned k = (bx - sc[lo].acc2_off) * 256u + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const double2 *p0 = part + sc[lo].part_off + k;
	double2 st = make_double2(0, 0), ps = make_double2(0, 0);
	if (carry_in) { st = cin[i]; ps = cinPS[i]; }
	for (unsigned b0 = 0; b0 < ntr; b0 += 4) { // four traces' loads in flight; the additions keep the step order
		double2 v[4];
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = p0[(size_t)(b0 + (unsigned)j < ntr ? b0 + (unsigned)j : ntr - 1u) * npart];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const unsigned b = b0 + (unsigned)j;
			if (b < ntr) {
				const unsigned cnt = steps[b].cnt;
				if (cnt == 1) { st = make_double2(0, 0); ps = make_double2(0, 0); }
				st.x += v[j].x; st.y += v[j].y;
				add_unit_phasor(ps, v[j]);
				OUT[(size_t)b * ncoef + i] = weight_value(st, ps, cnt == 1 ? mode1 : mode, (double)cnt, (double)cnt, wu);
			}
		}
	}
	if (carry_out) { cout[i] = st; coutPS[i] = ps; }
}

// Partial-stack rows of two-stage step blockIdx.y (Tr = steps[].cnt traces from the ensemble's first one), samples [256 blockIdx.x, + 256):
// row g = the FP64 sum, in trace order, of the traces j with floor(j KM / Tr) == g -- the contiguous range [ceil(g Tr / KM), ceil((g + 1) Tr / KM)),
// never empty (Tr > KM) -- to rows[(blockIdx.y KM + g) N + n].
__global__ void __launch_bounds__(256) k_cb_step_rows(const float *__restrict__ x, size_t ld, size_t N, size_t first0, const CbStep *__restrict__ steps,
                                                      unsigned KM, double *__restrict__ rows)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const CbStep s = steps[blockIdx.y];
	const unsigned Tr = s.cnt;
	const float *src = x + (first0 + s.dst + 1 - Tr) * ld + n;
	double *dst = rows + (size_t)blockIdx.y * KM * N + n;
	unsigned g = 0;
	unsigned long long e = ((unsigned long long)Tr + KM - 1) / KM; // end of group g
	double acc = 0;
	for (unsigned j0 = 0; j0 < Tr; j0 += 8) { // eight rows' loads in flight; the additions keep the trace order
		float v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = src[(size_t)(j0 + (unsigned)j < Tr ? j0 + (unsigned)j : Tr - 1u) * ld];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const unsigned t = j0 + (unsigned)j;
			if (t < Tr) {
				acc += (double)v[j];
				if (t + 1 == e) {
					dst[(size_t)g * N] = acc;
					acc = 0; g++;
					e = ((unsigned long long)(g + 1) * Tr + KM - 1) / KM;
				}
			}
		}
	}
}

// k_dot4 (resample.hip) with a reference row per reconstruction: row r of d against row steps[r].ens of ref; the four sums
// (sum d r, sum d d, sum (d - r)^2, sum r r) to out[steps[r].dst], the float cast of d to row steps[r].dst of `cast` when that is wanted.
// One workgroup per row, fixed order.
__global__ void __launch_bounds__(1024) k_cb_dot4(const double *__restrict__ d, const CbStep *__restrict__ steps, const float *__restrict__ ref, size_t N,
                                                  double *__restrict__ out, float *__restrict__ cast)
{
	const CbStep s = steps[blockIdx.x];
	d += (size_t)blockIdx.x * N;
	const float *r = ref + (size_t)s.ens * N;
	float *c = cast ? cast + (size_t)s.dst * N : nullptr;
	__shared__ double red[16][4];
	double a = 0, b = 0, q = 0, e = 0;
	for (size_t n = threadIdx.x; n < N; n += 1024) {
		const double dv = d[n], rv = (double)r[n], df = dv - rv;
		a = fma(dv, rv, a); b = fma(dv, dv, b); q = fma(df, df, q); e = fma(rv, rv, e);
		if (c) c[n] = (float)dv;
	}
	a = wave_sum(a); b = wave_sum(b); q = wave_sum(q); e = wave_sum(e);
	if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; red[threadIdx.x >> 6][2] = q; red[threadIdx.x >> 6][3] = e; }
	__syncthreads();
	if (threadIdx.x < 4) {
		double t = 0;
		for (int w = 0; w < 16; w++) t += red[w][threadIdx.x];
		out[(size_t)s.dst * 4 + threadIdx.x] = t;
	}
}

// sum ref[b][n]^2 of every reference row (the order of k_dot4's fourth sum)
__global__ void __launch_bounds__(1024) k_cb_refsq(const float *__restrict__ ref, size_t N, double *__restrict__ out)
{
	const float *r = ref + (size_t)blockIdx.x * N;
	__shared__ double red[16];
	double e = 0;
	for (size_t n = threadIdx.x; n < N; n += 1024) { const double rv = (double)r[n]; e = fma(rv, rv, e); }
	e = wave_sum(e);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
	__syncthreads();
	if (threadIdx.x == 0) {
		double t = 0;
		for (int w = 0; w < 16; w++) t += red[w];
		out[blockIdx.x] = t;
	}
}

// k_conv_linear (resample.hip) for ensemble blockIdx.y of a round: d += x_j; d *= (float)(1 / (j + 1)); metrics against the ensemble's
// reference row; steps; d *= (j + 1)   (:288-308), from zero for every ensemble.  The partial sums of workgroup blockIdx.x for entry
// e.off + j of the round go to partial[(blockIdx.x T + e.off + j) 3 ..]; k_cb_lin_reduce adds them in workgroup order.
__global__ void __launch_bounds__(256) k_cb_linear(const float *__restrict__ x, size_t ld, size_t N, const CbEns *__restrict__ ens, size_t T,
                                                   const float *__restrict__ ref, double *__restrict__ partial, float *__restrict__ steps)
{
	__shared__ double red[4][3];
	const CbEns e = ens[blockIdx.y];
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool live = n < N;
	const double rv = live ? (double)ref[(size_t)e.b * N + n] : 0.0;
	x += e.t0 * ld;
	double d = 0;
	for (size_t i = 0; i < e.m; i++) {
		if (live) d += (double)x[i * ld + n];
		const float inv = (float)(1.0 / (double)(i + 1));
		d *= (double)inv;
		const double df = d - rv;
		double a = live ? d * rv : 0.0, b = live ? d * d : 0.0, c = live ? df * df : 0.0;
		a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
		if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; red[threadIdx.x >> 6][2] = c; }
		__syncthreads();
		if (threadIdx.x < 3)
			partial[((size_t)blockIdx.x * T + e.off + i) * 3 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
		__syncthreads();
		if (steps && live) steps[((size_t)e.dst + i) * N + n] = (float)d;
		d *= (double)(i + 1);
	}
}

__global__ void __launch_bounds__(256) k_cb_lin_reduce(const double *__restrict__ partial, unsigned nblocks, size_t T, double *__restrict__ out)
{
	const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; // index into [T][3]
	if (j >= T * 3) return;
	double t = 0;
	for (unsigned b = 0; b < nblocks; b++) t += partial[(size_t)b * T * 3 + j];
	out[j] = t;
}

extern "C" int tspws_hip_convergence_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                                           const float *d_ref_ts, const float *d_ref_ls, double *h_ts_sim, double *h_ts_misfit, double *h_ls_sim,
                                           double *h_ls_misfit, float *d_ts_steps, float *d_ls_steps, void *s)
{
	// (the checks that need no plan come first: a host without a device can see every one of them refuse)
	if (!p || !h_first) return fail(TSPWS_E_ARG, "convergence_batch: NULL");
	if (!B) return pl ? 0 : fail(TSPWS_E_ARG, "convergence_batch: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "convergence_batch: decreasing ensemble offsets");
	const size_t first0 = h_first[0], Tn = h_first[B] - first0;
	if (Tn && (!d_x || !d_ref_ts || !d_ref_ls || !h_ts_sim || !h_ts_misfit || !h_ls_sim || !h_ls_misfit)) return fail(TSPWS_E_ARG, "convergence_batch: NULL");
	if (!pl) return fail(TSPWS_E_ARG, "convergence_batch: NULL");
	if (!Tn) return 0;
	const size_t N = pl->N, nc = pl->ncoef;
	if (ld < N) return fail(TSPWS_E_ARG, "convergence_batch: row stride below the trace length");
	if (Tn > 0xfffffff0ull) return fail(TSPWS_E_ARG, "convergence_batch: more than 2^32 traces");
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	const unsigned KM = p->Kmax;
	int rc;
	void *v;

	// the steps of both kinds, the ensembles
	std::vector<CbStep> inc, two;
	std::vector<CbEns> ens;
	for (unsigned b = 0; b < B; b++) {
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		if (!m) continue;
		const size_t n1 = KM ? std::min<size_t>(m, KM) : m;
		for (size_t j = 0; j < m; j++) {
			CbStep q;
			q.cnt = (unsigned)(j + 1); q.ens = b; q.dst = (unsigned)(f - first0 + j); q.pad = 0;
			(j < n1 ? inc : two).push_back(q);
		}
		CbEns e;
		e.t0 = f; e.m = (unsigned)m; e.b = b; e.dst = (unsigned)(f - first0); e.off = 0;
		ens.push_back(e);
	}
	tspws_hip_conv_batch_stats &stats = pl->conv_batch_stats;
	stats = tspws_hip_conv_batch_stats();
	stats.single_steps = (unsigned)inc.size();
	stats.two_stage_steps = (unsigned)two.size();
	stats.rows = (unsigned)(two.size() * KM);
	stats.empty = B - (unsigned)ens.size();
	if (ens.size() == 1) { // one ensemble: the single call
		const CbEns &e = ens[0];
		stats.looped = 1;
		return tspws_hip_convergence(pl, p, d_x + e.t0 * ld, ld, e.m, d_ref_ts + (size_t)e.b * N, d_ref_ls + (size_t)e.b * N, h_ts_sim + e.dst,
		                             h_ts_misfit + e.dst, h_ls_sim + e.dst, h_ls_misfit + e.dst, d_ts_steps ? d_ts_steps + (size_t)e.dst * N : nullptr,
		                             d_ls_steps ? d_ls_steps + (size_t)e.dst * N : nullptr, s);
	}

	// rounds: every block that grows with the steps within the budget
	const size_t budget = tspws_part_budget_bytes();
	const size_t per_set = std::max(pl->npart * sizeof(double2), tspws_inverse_row_bytes(pl));
	const size_t nI = inc.size(), n2 = two.size(), nE = ens.size();
	const size_t R1 = std::max<size_t>(1, std::min<size_t>({nI, budget / per_set, (size_t)65535 * (CB_CHAIN / 2)}));
	const size_t per_step2 = std::max({(size_t)KM * pl->npart * sizeof(double2), (size_t)KM * N * sizeof(double), 2 * nc * sizeof(double2), per_set});
	const size_t R2 = n2 ? std::max<size_t>(1, std::min<size_t>({n2, budget / per_step2, 65535, 0xfffffff0ull / KM})) : 0;
	// chains of the prefix walk: whole ensembles until a chain has CB_CHAIN steps; a round begins a chain (<= 65535 of them a round)
	std::vector<unsigned> chain;
	std::vector<size_t> chain0; // first chain of every round (+ the end)
	for (size_t q = 0; q < nI; q++) {
		const bool round_start = q % R1 == 0;
		if (round_start) chain0.push_back(chain.size());
		if (round_start || (inc[q].cnt == 1 && q - chain.back() >= CB_CHAIN)) chain.push_back((unsigned)q);
	}
	// (every round's chain list ends with the round's end: one entry more per round)
	std::vector<unsigned> chain_tab;
	std::vector<size_t> chain_at;
	for (size_t r = 0; r < chain0.size(); r++) {
		const size_t c0 = chain0[r], c1 = r + 1 < chain0.size() ? chain0[r + 1] : chain.size();
		chain_at.push_back(chain_tab.size());
		chain_tab.insert(chain_tab.end(), chain.begin() + c0, chain.begin() + c1);
		chain_tab.push_back((unsigned)std::min(nI, (r + 1) * R1));
	}
	chain_at.push_back(chain_tab.size());
	// rounds of the linear curve: whole ensembles whose partial sums fit
	const unsigned nblk = (unsigned)((N + 255) / 256);
	std::vector<size_t> toff(nE + 1, 0); // traces in front of ensemble e
	for (size_t e = 0; e < nE; e++) toff[e + 1] = toff[e] + ens[e].m;
	const std::vector<Round> lrounds = whole_ensemble_rounds(nE, [&](size_t e0, size_t e1) {
		return e1 - e0 <= 65535 && (toff[e1] - toff[e0]) * nblk * 3 * sizeof(double) <= budget;
	});
	size_t maxT = 0;
	for (const Round &lr : lrounds) {
		for (size_t e = lr.j0; e < lr.j1; e++) ens[e].off = (unsigned)(toff[e] - toff[lr.j0]);
		maxT = std::max(maxT, toff[lr.j1] - toff[lr.j0]);
	}

	// the tables, in one block: incremental steps | two-stage steps | ensembles | their trace counts (doubles) | chains
	TableLayout lay;
	const size_t o_inc = lay.add<CbStep>(nI), o_two = lay.add<CbStep>(n2), o_ens = lay.add<CbEns>(nE), o_mv = lay.add<double>(n2),
	             o_ch = lay.add<unsigned>(chain_tab.size()), tab_bytes = lay.bytes;
	if (tab_bytes > budget) return fail(TSPWS_E_ARG, "convergence_batch: the step tables (24 bytes a trace) exceed TSPWS_PART_MB");
	BatchCall call(st);
	char *blob = call.block(tab_bytes), *tab;
	if (nI) memcpy(blob + o_inc, inc.data(), nI * sizeof(CbStep));
	if (n2) memcpy(blob + o_two, two.data(), n2 * sizeof(CbStep));
	memcpy(blob + o_ens, ens.data(), nE * sizeof(CbEns));
	for (size_t q = 0; q < n2; q++) ((double *)(blob + o_mv))[q] = (double)two[q].cnt;
	memcpy(blob + o_ch, chain_tab.data(), chain_tab.size() * sizeof(unsigned));

	// scratch, all of it before the first launch
	const bool gather = KM != 0; // (without a two-stage rule the list is the trace array itself)
	const size_t Rm = std::max(R1, R2);
	if ((rc = scratch(pl, SCR_PART, std::max<size_t>(2, std::max(R1, R2 * KM)) * pl->npart * sizeof(double2), &v))) return rc;
	double2 *part = (double2 *)v;
	float *xg = nullptr;
	if (gather) { if ((rc = scratch(pl, SCR_CBX, R1 * N * sizeof(float), &v))) return rc; xg = (float *)v; }
	if ((rc = scratch(pl, SCR_ROWY, Rm * nc * sizeof(double2), &v))) return rc;
	double2 *OUT = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWX, Rm * N * sizeof(double), &v))) return rc;
	double *xr = (double *)v;
	if ((rc = scratch(pl, SCR_CBST, (R2 + 2) * 2 * nc * sizeof(double2), &v))) return rc;
	// the carried running pair twice (a round reads the one the last round wrote and writes the other: its first and last chain run side by
	// side), then a plane pair per two-stage step
	double2 *carry = (double2 *)v, *STr = carry + 4 * nc;
	double *rows = nullptr;
	if (n2) { if ((rc = scratch(pl, SCR_CBP, R2 * KM * N * sizeof(double), &v))) return rc; rows = (double *)v; }
	if ((rc = scratch(pl, SCR_CBM, (Tn * 7 + B + (size_t)nblk * maxT * 3) * sizeof(double), &v))) return rc;
	double *d_ts = (double *)v, *d_lin = d_ts + Tn * 4, *d_lsq = d_lin + Tn * 3, *d_lpart = d_lsq + B;

	if ((rc = call.upload(pl, SCR_BTAB, blob, tab_bytes, &tab))) return rc;
	const CbStep *d_inc = (const CbStep *)(tab + o_inc), *d_two = (const CbStep *)(tab + o_two);
	const CbEns *d_ens = (const CbEns *)(tab + o_ens);
	const double *d_Mv = (const double *)(tab + o_mv);
	const unsigned *d_chain = (const unsigned *)(tab + o_ch);

	// incremental steps
	const int mode = tspws_weight_mode(p->wu, p->unbiased, 2), mode1 = tspws_weight_mode(p->wu, p->unbiased, 1);
	for (size_t q0 = 0, r = 0; q0 < nI; q0 += R1, r++) {
		const size_t nb = std::min(R1, nI - q0);
		const unsigned nchain = (unsigned)(chain_at[r + 1] - chain_at[r] - 1);
		stats.rounds++;
		const float *xb = d_x + (first0 + q0) * ld;
		size_t ldb = ld;
		if (gather) {
			hipLaunchKernelGGL(k_cb_gather, dim3(nblk, (unsigned)std::min<size_t>(nb, 65535)), dim3(256), 0, st, d_x, ld, N, first0, d_inc + q0, xg);
			for (size_t g0 = 65535; g0 < nb; g0 += 65535)
				hipLaunchKernelGGL(k_cb_gather, dim3(nblk, (unsigned)std::min<size_t>(nb - g0, 65535)), dim3(256), 0, st, d_x, ld, N, first0, d_inc + q0 + g0, xg + g0 * N);
			xb = xg; ldb = N;
		}
		if ((rc = tspws_forward_parts<float>(pl, xb, nb, ldb, part, st, nullptr, ScaleRange()))) return rc;
		hipLaunchKernelGGL(k_cb_prefix, dim3(pl->acc2_blocks, nchain), dim3(256), 0, st, (const double2 *)part, pl->npart, (const ScaleDesc *)pl->d_sc, pl->S, d_inc,
		                   d_chain + chain_at[r], (unsigned)q0, OUT, nc, (const double2 *)carry + (r & 1) * 2 * nc, carry + ((r + 1) & 1) * 2 * nc, mode, mode1, p->wu);
		if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nb, xr, s))) return rc;
		hipLaunchKernelGGL(k_cb_dot4, dim3((unsigned)nb), dim3(1024), 0, st, (const double *)xr, d_inc + q0, d_ref_ts, N, d_ts, d_ts_steps);
	}

	// two-stage steps: Kmax rows a step, a stack per step
	const bool fuse = tspws_fused_forward(pl);
	for (size_t q0 = 0; q0 < n2; q0 += R2) {
		const size_t nb = std::min(R2, n2 - q0);
		stats.rounds++;
		hipLaunchKernelGGL(k_cb_step_rows, dim3(nblk, (unsigned)nb), dim3(256), 0, st, d_x, ld, N, first0, d_two + q0, KM, rows);
		FuseOut fz;
		fz.accST = STr; fz.accPS = STr + nc; fz.stride = 2 * nc; fz.tps = KM;
		if ((rc = tspws_forward_parts<double>(pl, rows, nb * KM, N, part, st, fuse ? &fz : nullptr, ScaleRange()))) return rc;
		WeightArgs wa;
		wa.OUT = OUT; wa.out_stride = nc; wa.mode = tspws_weight_mode(p->wu, p->unbiased, KM); wa.K = (double)KM; wa.wu = p->wu; wa.Mv = d_Mv + q0;
		tspws_launch_accumulate(pl, (const double2 *)part, KM, STr, STr + nc, 1, &fz, 1, st, (unsigned)nb, (size_t)KM * pl->npart, 2 * nc, nullptr, &wa, ScaleRange());
		if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nb, xr, s))) return rc;
		hipLaunchKernelGGL(k_cb_dot4, dim3((unsigned)nb), dim3(1024), 0, st, (const double *)xr, d_two + q0, d_ref_ts, N, d_ts, d_ts_steps);
	}

	// the linear curve
	for (const Round &lr : lrounds) {
		const size_t dst0 = ens[lr.j0].dst, T = toff[lr.j1] - toff[lr.j0];
		hipLaunchKernelGGL(k_cb_linear, dim3(nblk, (unsigned)(lr.j1 - lr.j0)), dim3(256), 0, st, d_x, ld, N, d_ens + lr.j0, T, d_ref_ls, d_lpart,
		                   d_ls_steps);
		hipLaunchKernelGGL(k_cb_lin_reduce, dim3((unsigned)((T * 3 + 255) / 256)), dim3(256), 0, st, (const double *)d_lpart, nblk, T, d_lin + dst0 * 3);
	}
	hipLaunchKernelGGL(k_cb_refsq, dim3(B), dim3(1024), 0, st, d_ref_ls, N, d_lsq);
	if (hipGetLastError() != hipSuccess) return fail(TSPWS_E_HIP, "convergence_batch: launch");

	// one copy per curve
	std::vector<double> hts(Tn * 4), hl(Tn * 3), lsq(B);
	hipError_t e1 = hipMemcpyAsync(hts.data(), d_ts, Tn * 4 * sizeof(double), hipMemcpyDeviceToHost, st);
	hipError_t e2 = hipMemcpyAsync(hl.data(), d_lin, Tn * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
	hipError_t e3 = hipMemcpyAsync(lsq.data(), d_lsq, B * sizeof(double), hipMemcpyDeviceToHost, st);
	hipError_t e4 = call.drain();
	for (hipError_t e : {e1, e2, e3, e4})
		if (e != hipSuccess) return fail(TSPWS_E_HIP, "convergence_batch: copy to the host", e);
	for (const CbEns &e : ens)
		for (size_t i = e.dst; i < (size_t)e.dst + e.m; i++) {
			h_ts_sim[i] = hts[i * 4] / sqrt(hts[i * 4 + 1]) / sqrt(hts[i * 4 + 3]);
			h_ts_misfit[i] = hts[i * 4 + 2];
			h_ls_sim[i] = hl[i * 3] / sqrt(hl[i * 3 + 1]) / sqrt(lsq[e.b]);
			h_ls_misfit[i] = hl[i * 3 + 2];
		}
	return 0;
}

extern "C" int tspws_hip_convergence_batch_stats(const tspws_hip_plan *pl, tspws_hip_conv_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "convergence_batch_stats: NULL");
	*stats = pl->conv_batch_stats;
	return 0;
}
