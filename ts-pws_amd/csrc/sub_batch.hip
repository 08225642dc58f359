// sub_batch.hip -- random subsamples of many ensembles in one call (tspws_hip_subsample_batch, tspws_hip_subsample_batch_sel).
// Reference citations are relative to the reference project's src/ directory.
//
// tspws_hip_subsample_sel gives the M random subsamples of ONE ensemble: per call a mask upload, a memset, a forward launch over a few dozen
// traces, k_accumulate_masked, k_sub_linear, a weight launch, an inverse over M rows, an epilogue and a wait.  The batched jackknives cannot
// stand in: under random masks nearly every trace is a selection class of its own (jk_batch.hip pads every class to a 64-trace block), and
// the single-stage subsampling body forms its linear rows with a FLOAT accumulator (ts_pws1f_lib.c:538-542).  This unit does the batch at once;
// every ensemble follows the single call's rule on its own size (two-stage iff 0 < Kmax <= M_b), and a batch may mix both kinds.
//   host       K_{b,m} of every (ensemble, mask); the ensembles with traces in two lists, single-stage and two-stage
//   single     rounds of whole ensembles.  The round's traces are transformed once (tspws_forward_parts, ONE call per stretch of contiguous
//              traces: two-stage ensembles in between cut a stretch, empty ones do not) into per-trace partials; k_sb_accumulate (coefficient
//              tile x group of 8 masks x ensemble) walks an ensemble's traces in trace order, sums each over its splits, normalises it once
//              and adds it to the register-held stacks of the masks that keep it -- the arithmetic of k_accumulate_masked (resample.hip), with
//              the 8 mask bits of a trace in one byte (one wave-uniform load per trace) and every ST / PS plane written exactly once, zero
//              planes included: no memset, no read-modify-write; k_sb_linear (sample tile x mask x ensemble): k_sub_linear's float accumulator;
//              then, per batch of rows that fits, k_sb_weight with each row's own K (K = M = K_{b,m}; the mode per row), one tspws_hip_inverse
//              and k_sb_epilogue, which scatters the float rows to [b][m]
//   two-stage  the shared walk of jk_batch_two_stage.hip over that list, without main rows (tspws_jb2_shared; its own rounds)
// Rounds keep every block that grows with the ensembles -- partials, plane pairs, weighted sets, reconstructions, the inverse's octave buffer,
// tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble, one ensemble alone may exceed it.  A batch with ONE
// non-empty ensemble is tspws_hip_subsample_sel for it (a single-stage one: when every row has the K that call derives from subsmpl_p).
// Nothing is atomic; every output has one writer and every sum a fixed order.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

#define is_two_stage tspws_is_two_stage

// (SbEns, the descriptor of a single-stage ensemble of a round, and the rows' finish -- k_sb_weight, k_sb_epilogue -- are in batch_kernels.h:
// boot_batch.hip runs them too)

// ST / PS planes of the masks 8 g .. 8 g + 7 (g = g0 + blockIdx.y) of ensemble blockIdx.z of the round, one thread per coefficient (the
// geometry of k_accumulate_masked: 256-coefficient blocks by acc_off).  Row r = blockIdx.z M + mask: planes[r][ST | PS], 2 ncoef apart.
__global__ void __launch_bounds__(256) k_sb_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                       size_t ncoef, const SbEns *__restrict__ ens, const unsigned char *__restrict__ bits, unsigned M,
                                                       unsigned g0, double2 *__restrict__ planes)
{
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, false);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	const unsigned k = (blockIdx.x - sc[lo].acc_off) * 256 + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const SbEns e = ens[blockIdx.z];
	const unsigned g = g0 + blockIdx.y, m0 = g * 8u, nm = (M - m0) < 8u ? (M - m0) : 8u, ntr = e.m;
	const unsigned char *bt = bits + e.bits_off + (size_t)g * ntr;
	const double2 *p0 = part + (size_t)e.part0 * npart + sc[lo].part_off + k;
	double2 st[8], ps[8];
#pragma unroll
	for (int m = 0; m < 8; m++) { st[m] = make_double2(0, 0); ps[m] = make_double2(0, 0); }
	for (unsigned b0 = 0; b0 < ntr; b0 += 4) { // four traces at a time: their loads are independent, the additions stay in trace order
		double2 a[4], u[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			a[j] = make_double2(0, 0);
			if (b0 + (unsigned)j < ntr) a[j] = p0[(size_t)(b0 + (unsigned)j) * npart];
		}
		for (unsigned sp = 1; sp < nsplit; sp++) {
			double2 t[4];
#pragma unroll
			for (int j = 0; j < 4; j++) t[j] = (b0 + (unsigned)j < ntr) ? p0[(size_t)(b0 + (unsigned)j) * npart + (size_t)sp * Ns] : make_double2(0, 0);
#pragma unroll
			for (int j = 0; j < 4; j++) { a[j].x += t[j].x; a[j].y += t[j].y; }
		}
#pragma unroll
		for (int j = 0; j < 4; j++) { u[j] = make_double2(0, 0); add_unit_phasor(u[j], a[j]); }
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (b0 + (unsigned)j < ntr) {
				const unsigned mb = (unsigned)__builtin_amdgcn_readfirstlane((int)bt[b0 + (unsigned)j]); // the trace's 8 mask bits (bits past M are zero)
#pragma unroll
				for (int m = 0; m < 8; m++) {
					if ((mb >> m) & 1u) { // (wave-uniform)
						st[m].x += a[j].x; st[m].y += a[j].y; ps[m].x += u[j].x; ps[m].y += u[j].y;
					}
				}
			}
		}
	}
	double2 *o = planes + ((size_t)blockIdx.z * M + m0) * 2 * ncoef + i;
#pragma unroll
	for (int m = 0; m < 8; m++)
		if ((unsigned)m < nm) { o[(size_t)m * 2 * ncoef] = st[m]; o[(size_t)m * 2 * ncoef + ncoef] = ps[m]; }
}

// time-domain linear stack of mask q0 + blockIdx.y of ensemble blockIdx.z: the reference's FLOAT accumulator over the kept traces in trace
// order (ts_pws1f_lib.c:538-542), then the float scale 1/K (:579-583) -- k_sub_linear (resample.hip) per (mask, ensemble); K = 0: a zero row
__global__ void __launch_bounds__(256) k_sb_linear(const float *__restrict__ x, size_t ld, size_t N, const SbEns *__restrict__ ens,
                                                   const unsigned char *__restrict__ bits, const unsigned *__restrict__ Kc, unsigned M, unsigned q0,
                                                   float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const SbEns e = ens[blockIdx.z];
	const unsigned q = q0 + blockIdx.y, K = Kc[(size_t)blockIdx.z * M + q], sh = q & 7u;
	float *o = out + ((size_t)e.row * M + q) * N;
	if (!K) { o[n] = 0.f; return; }
	const unsigned char *row = bits + e.bits_off + (size_t)(q >> 3) * e.m;
	const float *xe = x + (size_t)e.t0 * ld + n;
	const size_t mtr = e.m;
	float acc = 0.f;
	for (size_t i0 = 0; i0 < mtr; i0 += 8) { // eight rows' loads in flight; the additions keep the trace order
		float v[8];
		bool on[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			on[j] = i0 + (size_t)j < mtr && ((row[i0 + (size_t)j] >> sh) & 1u); // (wave-uniform)
			v[j] = on[j] ? xe[(i0 + (size_t)j) * ld] : 0.f;
		}
#pragma unroll
		for (int j = 0; j < 8; j++)
			if (on[j]) acc = (float)((double)acc + (double)v[j]);
	}
	o[n] = acc * (float)(1. / (double)K);
}

namespace {

struct Ens { unsigned b; size_t f, m; }; // ensemble with traces: index, first trace, traces

// the tables of a round in one block: ensembles | K of every row | mask bytes
struct SbTab { size_t ens, kc, bits, bytes; };
SbTab sb_tab(size_t ne, size_t nrows, size_t nbits)
{
	TableLayout lay;
	const size_t ens = lay.add<SbEns>(ne), kc = lay.add<unsigned>(nrows), bits = lay.add<unsigned char>(nbits);
	return {ens, kc, bits, lay.bytes};
}

// the single-stage ensembles E of the batch in rounds
int single_rounds(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t first0, const std::vector<Ens> &E, unsigned M, const char *h_sel,
                  size_t Tn, float *d_ls_out, float *d_ts_out, const unsigned *h_Kc, BatchCall &call)
{
	const size_t N = pl->N, nc = pl->ncoef, n = E.size(), budget = tspws_part_budget_bytes();
	hipStream_t st = call.stream();
	const unsigned ng = (M + 7) / 8;
	int rc;
	void *v;
	// rounds of whole ensembles: the partials of their traces, a plane pair per (ensemble, mask) and the tables within the budget; ensembles
	// within grid.z, partial indices and rows within 32 bits
	std::vector<size_t> tr0(n + 1, 0); // traces in front of ensemble j
	for (size_t j = 0; j < n; j++) tr0[j + 1] = tr0[j] + E[j].m;
	auto tab_of = [&](size_t j0, size_t j1) { return sb_tab(j1 - j0, (j1 - j0) * M, (tr0[j1] - tr0[j0]) * ng); };
	const std::vector<Round> rounds = whole_ensemble_rounds(n, [&](size_t j0, size_t j1) {
		const size_t ne = j1 - j0, nt = tr0[j1] - tr0[j0];
		return !(ne > 65535 || ne * M > 0xfffffff0ull || nt > 0xfffffff0ull || nt * pl->npart * sizeof(double2) > budget || ne * M * 2 * nc * sizeof(double2) > budget ||
		         tab_of(j0, j1).bytes > budget);
	});
	size_t max_ntr = 0, max_ne = 0, max_tab = 0;
	for (const Round &r : rounds) {
		max_ntr = std::max(max_ntr, tr0[r.j1] - tr0[r.j0]);
		max_ne = std::max(max_ne, r.j1 - r.j0);
		max_tab = std::max(max_tab, tab_of(r.j0, r.j1).bytes);
	}
	if (max_ntr > 0xfffffff0ull || max_ne * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "subsample_batch: more than 2^32 traces or mask rows in one ensemble");
	// rows per finish batch
	const size_t RB = even_rows_per_batch(budget, tspws_inverse_row_bytes(pl), max_ne * M);
	if ((rc = scratch(pl, SCR_PART, std::max<size_t>(2, max_ntr) * pl->npart * sizeof(double2), &v))) return rc;
	double2 *part = (double2 *)v;
	if ((rc = scratch(pl, SCR_SBPL, max_ne * M * 2 * nc * sizeof(double2), &v))) return rc;
	double2 *planes = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWY, RB * nc * sizeof(double2), &v))) return rc;
	double2 *OUT = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWX, RB * N * sizeof(double), &v))) return rc;
	double *xr = (double *)v;
	const unsigned nb256 = (unsigned)((N + 255) / 256);

	for (const Round &r : rounds) {
		const size_t ne = r.j1 - r.j0, nrows = ne * M;
		pl->sub_batch_stats.rounds++;
		// the round's tables (here the counts are the round's own: the bound holds with equality)
		const SbTab o = tab_of(r.j0, r.j1);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, "subsample_batch: table bound"); // (cannot happen)
		char *blob = call.block(o.bytes), *tab;
		SbEns *he = (SbEns *)(blob + o.ens);
		unsigned *hkc = (unsigned *)(blob + o.kc);
		unsigned char *hb = (unsigned char *)(blob + o.bits);
		size_t t = 0;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = E[j];
			SbEns d;
			d.t0 = e.f; d.bits_off = t * ng; d.m = (unsigned)e.m; d.part0 = (unsigned)t; d.row = e.b; d.pad = 0;
			he[j - r.j0] = d;
			memcpy(hkc + (j - r.j0) * (size_t)M, h_Kc + (size_t)e.b * M, (size_t)M * 4);
			unsigned char *eb = hb + d.bits_off; // (zero so far)
			for (unsigned q = 0; q < M; q++) {
				const char *row = h_sel + (size_t)q * Tn + (e.f - first0);
				unsigned char *dst = eb + (size_t)(q >> 3) * e.m;
				const unsigned char bit = (unsigned char)(1u << (q & 7u));
				for (size_t i = 0; i < e.m; i++) if (row[i] == 1) dst[i] |= bit;
			}
			t += e.m;
		}
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const SbEns *d_ens = (const SbEns *)(tab + o.ens);
		const unsigned *d_kc = (const unsigned *)(tab + o.kc);
		const unsigned char *d_bits = (const unsigned char *)(tab + o.bits);

		// every trace of the round once: a forward call per stretch of contiguous traces
		for (size_t j = r.j0; j < r.j1;) {
			size_t k = j + 1, nt = E[j].m;
			while (k < r.j1 && E[k].f == E[k - 1].f + E[k - 1].m) nt += E[k++].m;
			if ((rc = tspws_forward_parts<float>(pl, d_x + E[j].f * ld, nt, ld, part + (size_t)he[j - r.j0].part0 * pl->npart, st, nullptr, ScaleRange()))) return rc;
			j = k;
		}
		for (unsigned g0 = 0; g0 < ng; g0 += 65535)
			hipLaunchKernelGGL(k_sb_accumulate, dim3(pl->acc_blocks, std::min(65535u, ng - g0), (unsigned)ne), dim3(256), 0, st, (const double2 *)part, pl->npart,
			                   (const ScaleDesc *)pl->d_sc, pl->S, nc, d_ens, d_bits, M, g0, planes);
		for (unsigned q0 = 0; q0 < M; q0 += 65535)
			hipLaunchKernelGGL(k_sb_linear, dim3(nb256, std::min(65535u, M - q0), (unsigned)ne), dim3(256), 0, st, d_x, ld, N, d_ens, d_bits, d_kc, M, q0, d_ls_out);
		// finish: the rows of the round in even batches
		for (size_t r0 = 0; r0 < nrows; r0 += RB) {
			const unsigned nr = (unsigned)std::min(RB, nrows - r0);
			hipLaunchKernelGGL(k_sb_weight, dim3((unsigned)((nc + 255) / 256), nr), dim3(256), 0, st, OUT, (const double2 *)planes, nc, d_kc, r0, p->wu, p->unbiased);
			if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nr, xr, (void *)st))) return rc;
			hipLaunchKernelGGL(k_sb_epilogue, dim3(nb256, nr), dim3(256), 0, st, (const double *)xr, N, d_ens, d_kc, M, r0, d_ts_out);
		}
	}
	return 0;
}

// what both entries refuse, in the order of the other batch calls: first what needs no plan.  *done: nothing to do (B == 0 or M == 0)
int check_args(const tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M, bool sel_ok,
               const float *d_ls_out, const float *d_ts_out, const unsigned *h_mtr_out, bool *done)
{
	*done = false;
	if (!p || !h_first) return fail(TSPWS_E_ARG, "subsample_batch: NULL");
	if (!B || !M) { *done = true; return pl ? 0 : fail(TSPWS_E_ARG, "subsample_batch: NULL"); }
	if (!sel_ok || !d_ls_out || !d_ts_out || !h_mtr_out) return fail(TSPWS_E_ARG, "subsample_batch: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "subsample_batch: decreasing ensemble offsets");
	bool two = false;
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m > 0xfffffff0ull) return fail(TSPWS_E_ARG, "subsample_batch: more than 2^32 traces in an ensemble");
		two |= m && is_two_stage(p, m);
	}
	if (two && ((size_t)M + 2 > 65535 || (size_t)M * p->Kmax > 0xffffffffull))
		return fail(TSPWS_E_ARG, "subsample_batch: too many masks for two-stage ensembles (M + 2 <= 65535, M Kmax < 2^32)");
	if (!pl) return fail(TSPWS_E_ARG, "subsample_batch: NULL");
	const size_t Tn = h_first[B] - h_first[0];
	if (Tn && !d_x) return fail(TSPWS_E_ARG, "subsample_batch: NULL traces");
	if (Tn && ld < pl->N) return fail(TSPWS_E_ARG, "subsample_batch: row stride below the trace length");
	return 0;
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
			if ((rc = single_rounds(pl, p, d_x, ld, first0, single, M, h_sel, Tn, d_ls_out, d_ts_out, h_mtr_out, call))) return rc;
		}
		if (!two.empty()) {
			stats.two_stage_shared = (unsigned)two.size();
			// (single_rounds has enqueued every round and kept no pointer: the walk may size the shared slots -- tables, sets, reconstructions -- anew)
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
