// boot_batch.hip -- bootstrap replicas of many ensembles in one call (tspws_hip_bootstrap_batch, tspws_hip_bootstrap_batch_cnt) and the host draw
// (tspws_bootstrap_plan, tspws_bootstrap_plan_batch).  Reference citations are relative to the reference project's src/ directory.
//
// A bootstrap replica draws M_b traces of an ensemble WITH replacement: a trace enters it 0, 1, 2, .. times, which no 0/1 selection can say.
// Replica (b, m) here is the single-stage resampling body (tspws_subsmpl_float, ts_pws1f_lib.c:501-610) with an all-ones mask on the EXPANDED
// ensemble -- the traces of ensemble b in trace order, trace i repeated cnt[m][i] times -- without ever forming that ensemble: the linear and
// phase stacks are sums over traces, so multiplicity only says how often a trace's coefficient and unit phasor are added.  The unit is the
// single-stage half of sub_batch.hip with one count byte per (replica, trace) in place of one mask bit:
//   host       K_{b,m} = the counts of row m inside ensemble b; rounds of whole ensembles
//   per round  the round's traces are transformed once (tspws_forward_parts, ONE call per stretch of contiguous traces) into per-trace partials;
//              k_bt_accumulate (coefficient tile x group of 8 replicas x ensemble) walks an ensemble's traces in trace order, sums each over its
//              splits, normalises it once and adds coefficient and phasor cnt times -- repeated addition, the order of operations of the
//              expanded ensemble -- to the register-held stacks of the 8 replicas (the 8 counts of a trace: one aligned 8-byte word, one
//              wave-uniform load); every ST / PS plane is written exactly once, zero planes included: no memset, no read-modify-write;
//              k_bt_linear (sample tile x replica x ensemble): the float accumulator of :538-542, once per copy; then, per batch of rows that
//              fits, k_sb_weight with each row's own K (K = M = K_{b,m}; the mode per row), one tspws_hip_inverse and k_sb_epilogue (the rows'
//              finish of sub_batch.hip, batch_kernels.h); k_bt_moments (sample tile x ensemble): mean and standard error over the replicas
// A 0/1 count row runs exactly the arithmetic of k_sb_accumulate / k_sb_linear on the same mask.  Two-stage ensembles are refused: in the
// expanded ensemble the group of a copy is floor(k Kmax / K), so a repeated trace can straddle group borders, which needs a walk of its own.
// Rounds keep every block that grows with the ensembles -- partials, plane pairs, weighted sets, reconstructions, the inverse's octave buffer,
// tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble, one ensemble alone may exceed it.  Nothing is atomic;
// every output has one writer and every sum a fixed order.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

// ST / PS planes of the replicas 8 g .. 8 g + 7 (g = g0 + blockIdx.y) of ensemble blockIdx.z of the round, one thread per coefficient (the
// geometry of k_sb_accumulate: 256-coefficient blocks by acc_off).  Row r = blockIdx.z M + replica: planes[r][ST | PS], 2 ncoef apart.
// cnt8[e.bits_off + g m + j]: byte q = how often trace j enters replica 8 g + q (replicas past M: zero).
__global__ void __launch_bounds__(256) k_bt_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                       size_t ncoef, const SbEns *__restrict__ ens, const unsigned long long *__restrict__ cnt8, unsigned M,
                                                       unsigned g0, double2 *__restrict__ planes)
{
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, false);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	const unsigned k = (blockIdx.x - sc[lo].acc_off) * 256 + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const SbEns e = ens[blockIdx.z];
	const unsigned g = g0 + blockIdx.y, m0 = g * 8u, nm = (M - m0) < 8u ? (M - m0) : 8u, ntr = e.m;
	const unsigned long long *ct = cnt8 + e.bits_off + (size_t)g * ntr;
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
				const unsigned long long w = ct[b0 + (unsigned)j]; // the trace's 8 counts
				const unsigned w0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w), w1 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w >> 32));
#pragma unroll
				for (int m = 0; m < 8; m++) {
					const unsigned c = ((m < 4 ? w0 : w1) >> (8 * (m & 3))) & 255u; // (wave-uniform)
					for (unsigned r = 0; r < c; r++) { // one addition per copy
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

// time-domain linear stack of replica q0 + blockIdx.y of ensemble blockIdx.z: the reference's FLOAT accumulator over the copies of the expanded
// ensemble in trace order (ts_pws1f_lib.c:538-542), one addition per copy, then the float scale 1/K (:579-583) -- k_sb_linear with counts;
// K = 0: a zero row.  cnt: the count words as bytes.
__global__ void __launch_bounds__(256) k_bt_linear(const float *__restrict__ x, size_t ld, size_t N, const SbEns *__restrict__ ens,
                                                   const unsigned char *__restrict__ cnt, const unsigned *__restrict__ Kc, unsigned M, unsigned q0,
                                                   float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const SbEns e = ens[blockIdx.z];
	const unsigned q = q0 + blockIdx.y, K = Kc[(size_t)blockIdx.z * M + q];
	float *o = out + ((size_t)e.row * M + q) * N;
	if (!K) { o[n] = 0.f; return; }
	const unsigned char *row = cnt + (e.bits_off + (size_t)(q >> 3) * e.m) * 8 + (q & 7u);
	const float *xe = x + (size_t)e.t0 * ld + n;
	const size_t mtr = e.m;
	float acc = 0.f;
	for (size_t i0 = 0; i0 < mtr; i0 += 8) { // eight rows' loads in flight (every row is loaded: no branch around a load); the additions keep the trace order
		float v[8];
		unsigned c[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const size_t t = i0 + (size_t)j < mtr ? i0 + (size_t)j : mtr - 1;
			v[j] = xe[t * ld];
			c[j] = i0 + (size_t)j < mtr ? row[t * 8] : 0u; // (wave-uniform)
		}
#pragma unroll
		for (int j = 0; j < 8; j++)
			for (unsigned r = 0; r < c[j]; r++) acc = (float)((double)acc + (double)v[j]);
	}
	o[n] = acc * (float)(1. / (double)K);
}

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

namespace {

struct Ens { unsigned b; size_t f, m; }; // ensemble with traces: index, first trace, traces

// the tables of a round in one block: ensembles | K of every row | count words
struct BtTab { size_t ens, kc, cnt, bytes; };
BtTab bt_tab(size_t ne, size_t nrows, size_t nwords)
{
	TableLayout lay;
	const size_t ens = lay.add<SbEns>(ne), kc = lay.add<unsigned>(nrows), cnt = lay.add<unsigned long long>(nwords);
	return {ens, kc, cnt, lay.bytes};
}

// the ensembles E of the batch in rounds
int rounds_of(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t first0, const std::vector<Ens> &E, unsigned M, const unsigned char *h_cnt,
              size_t Tn, float *d_ls_out, float *d_ts_out, const unsigned *h_Kc, float *d_stats, BatchCall &call)
{
	const size_t N = pl->N, nc = pl->ncoef, n = E.size(), budget = tspws_part_budget_bytes();
	hipStream_t st = call.stream();
	const unsigned ng = (M + 7) / 8;
	int rc;
	void *v;
	// rounds of whole ensembles: the partials of their traces, a plane pair per (ensemble, replica) and the tables within the budget; ensembles
	// within grid.z (grid.y of the moments), partial indices and rows within 32 bits
	std::vector<size_t> tr0(n + 1, 0); // traces in front of ensemble j
	for (size_t j = 0; j < n; j++) tr0[j + 1] = tr0[j] + E[j].m;
	auto tab_of = [&](size_t j0, size_t j1) { return bt_tab(j1 - j0, (j1 - j0) * M, (tr0[j1] - tr0[j0]) * ng); };
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
	if (max_ntr > 0xfffffff0ull || max_ne * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "bootstrap_batch: more than 2^32 traces or replica rows in one ensemble");
	// rows per finish batch
	const size_t RB = even_rows_per_batch(budget, tspws_inverse_row_bytes(pl), max_ne * M);
	// (SCR_SBPL: the plane pairs of whichever of sub_batch.hip / boot_batch.hip is running; neither keeps a pointer across calls)
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
		pl->boot_batch_stats.rounds++;
		// the round's tables (here the counts are the round's own: the bound holds with equality)
		const BtTab o = tab_of(r.j0, r.j1);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, "bootstrap_batch: table bound"); // (cannot happen)
		char *blob = call.block(o.bytes), *tab;
		SbEns *he = (SbEns *)(blob + o.ens);
		unsigned *hkc = (unsigned *)(blob + o.kc);
		unsigned char *hc = (unsigned char *)(blob + o.cnt);
		size_t t = 0;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = E[j];
			SbEns d;
			d.t0 = e.f; d.bits_off = t * ng; d.m = (unsigned)e.m; d.part0 = (unsigned)t; d.row = e.b; d.pad = 0;
			he[j - r.j0] = d;
			memcpy(hkc + (j - r.j0) * (size_t)M, h_Kc + (size_t)e.b * M, (size_t)M * 4);
			unsigned char *eb = hc + d.bits_off * 8; // (zero so far)
			for (unsigned q = 0; q < M; q++) {
				const unsigned char *row = h_cnt + (size_t)q * Tn + (e.f - first0);
				unsigned char *dst = eb + (size_t)(q >> 3) * e.m * 8 + (q & 7u);
				for (size_t i = 0; i < e.m; i++) dst[i * 8] = row[i];
			}
			t += e.m;
		}
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const SbEns *d_ens = (const SbEns *)(tab + o.ens);
		const unsigned *d_kc = (const unsigned *)(tab + o.kc);
		const unsigned long long *d_cnt = (const unsigned long long *)(tab + o.cnt);

		// every trace of the round once: a forward call per stretch of contiguous traces (empty ensembles in between do not cut a stretch)
		for (size_t j = r.j0; j < r.j1;) {
			size_t k = j + 1, nt = E[j].m;
			while (k < r.j1 && E[k].f == E[k - 1].f + E[k - 1].m) nt += E[k++].m;
			if ((rc = tspws_forward_parts<float>(pl, d_x + E[j].f * ld, nt, ld, part + (size_t)he[j - r.j0].part0 * pl->npart, st, nullptr, ScaleRange()))) return rc;
			j = k;
		}
		for (unsigned g0 = 0; g0 < ng; g0 += 65535)
			hipLaunchKernelGGL(k_bt_accumulate, dim3(pl->acc_blocks, std::min(65535u, ng - g0), (unsigned)ne), dim3(256), 0, st, (const double2 *)part, pl->npart,
			                   (const ScaleDesc *)pl->d_sc, pl->S, nc, d_ens, d_cnt, M, g0, planes);
		for (unsigned q0 = 0; q0 < M; q0 += 65535)
			hipLaunchKernelGGL(k_bt_linear, dim3(nb256, std::min(65535u, M - q0), (unsigned)ne), dim3(256), 0, st, d_x, ld, N, d_ens, (const unsigned char *)d_cnt, d_kc,
			                   M, q0, d_ls_out);
		// finish: the rows of the round in even batches
		for (size_t r0 = 0; r0 < nrows; r0 += RB) {
			const unsigned nr = (unsigned)std::min(RB, nrows - r0);
			hipLaunchKernelGGL(k_sb_weight, dim3((unsigned)((nc + 255) / 256), nr), dim3(256), 0, st, OUT, (const double2 *)planes, nc, d_kc, r0, p->wu, p->unbiased);
			if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nr, xr, (void *)st))) return rc;
			hipLaunchKernelGGL(k_sb_epilogue, dim3(nb256, nr), dim3(256), 0, st, (const double *)xr, N, d_ens, d_kc, M, r0, d_ts_out);
		}
		// the statistic over the replicas, from the float rows the round has just written
		if (d_stats)
			hipLaunchKernelGGL(k_bt_moments, dim3(nb256, (unsigned)ne), dim3(256), 0, st, (const float *)d_ls_out, (const float *)d_ts_out, N, d_ens, d_kc, M, d_stats);
	}
	return 0;
}

// what both entries refuse, in the order of the other batch calls: first what needs no plan.  *done: nothing to do (B == 0 or M == 0)
int check_args(const tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M, bool cnt_ok,
               const float *d_ls_out, const float *d_ts_out, const unsigned *h_mtr_out, bool *done)
{
	*done = false;
	if (!p || !h_first) return fail(TSPWS_E_ARG, "bootstrap_batch: NULL");
	if (!B || !M) { *done = true; return pl ? 0 : fail(TSPWS_E_ARG, "bootstrap_batch: NULL"); }
	if (!cnt_ok || !d_ls_out || !d_ts_out || !h_mtr_out) return fail(TSPWS_E_ARG, "bootstrap_batch: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "bootstrap_batch: decreasing ensemble offsets");
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m > 0xfffffff0ull) return fail(TSPWS_E_ARG, "bootstrap_batch: more than 2^32 traces in an ensemble");
		if (m && tspws_is_two_stage(p, m))
			return fail(TSPWS_E_ARG, "bootstrap_batch: a two-stage ensemble (0 < Kmax <= its traces): the two-stage bootstrap is not built, only single-stage ensembles");
	}
	if (!pl) return fail(TSPWS_E_ARG, "bootstrap_batch: NULL");
	const size_t Tn = h_first[B] - h_first[0];
	if (Tn && !d_x) return fail(TSPWS_E_ARG, "bootstrap_batch: NULL traces");
	if (Tn && ld < pl->N) return fail(TSPWS_E_ARG, "bootstrap_batch: row stride below the trace length");
	return 0;
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
	if (!E.empty() && (rc = rounds_of(pl, p, d_x, ld, first0, E, M, h_cnt, Tn, d_ls_out, d_ts_out, h_mtr_out, d_stats, call))) return rc;
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
