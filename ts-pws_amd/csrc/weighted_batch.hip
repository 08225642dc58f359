// weighted_batch.hip -- real-weighted stacks of many ensembles in one call (tspws_hip_weighted_stack_batch).  Reference citations are relative
// to the reference project's src/ directory.
//
// The reference's linear stack takes a weight per trace (tspws_stacks_float, ts_pws1f_lib.c:485-490) that nothing ever passes and that leaves the
// phase stack and the normalisers unweighted.  Row (b, m) here is the consistent form: with w_i >= 0 the weights of row m on the traces of
// ensemble b, n+ the traces with w_i > 0, W = sum w_i, Q = sum w_i^2 and Keff = W W / Q,
//   ST = sum w_i Y_i, PS = sum w_i Y_i / |Y_i|, coherence c = |PS| / W, bias of c^2 for random phases = Q / W^2 = 1 / Keff.
// The unit is the third sibling of sub_batch.hip (one mask bit per (row, trace)) and boot_batch.hip (one count byte): one FP64 weight.
//   host       n+, W, Q, Keff of every row (FP64, trace order); rounds of whole ensembles
//   per round  the round's traces are transformed once (tspws_forward_parts, ONE call per stretch of contiguous traces) into per-trace partials;
//              k_wb_accumulate (coefficient tile x group of 8 rows x ensemble) walks an ensemble's traces in trace order, sums each over its
//              splits, normalises it once and adds w times coefficient and phasor -- one fused multiply-add per component -- to the
//              register-held stacks of the 8 rows (the 8 weights of a trace: one aligned 64-byte block, read through a wave-uniform address;
//              a zero weight skips the trace); every ST / PS plane is written exactly once, zero planes included: no memset, no
//              read-modify-write; k_wb_linear (sample tile x row x ensemble): the float accumulator of :538-542 with the addend w x; then, per
//              batch of rows that fits, k_wb_weight with each row's (n+, W, Keff), one tspws_hip_inverse and k_sb_epilogue (batch_kernels.h)
// A 0/1 row runs exactly the arithmetic of k_sb_accumulate / k_sb_linear on the same mask (fma(1, a, s) = s + a), and W = Keff = K gives
// weight_value(K, K).  Two-stage ensembles are refused by design: with real weights the groups floor(k Kmax / K) have no meaning.
// Rounds keep every block that grows with the ensembles -- partials, plane pairs, weighted sets, reconstructions, the inverse's octave buffer,
// tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble, one ensemble alone may exceed it.  Nothing is atomic;
// every output has one writer and every sum a fixed order.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

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

// ST / PS planes of the rows 8 g .. 8 g + 7 (g = g0 + blockIdx.y) of ensemble blockIdx.z of the round, one thread per coefficient (the
// geometry of k_bt_accumulate).  Row r = blockIdx.z M + row: planes[r][ST | PS], 2 ncoef apart.  w8[e.bits_off + g m + j]: the 8 weights of trace j.
__global__ void __launch_bounds__(256) k_wb_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                       size_t ncoef, const SbEns *__restrict__ ens, const Wb8 *__restrict__ w8, unsigned M, unsigned g0,
                                                       double2 *__restrict__ planes)
{
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, false);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	const unsigned k = (blockIdx.x - sc[lo].acc_off) * 256 + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const SbEns e = ens[blockIdx.z];
	const unsigned g = g0 + blockIdx.y, m0 = g * 8u, nm = (M - m0) < 8u ? (M - m0) : 8u, ntr = e.m;
	const Wb8 *wt = w8 + e.bits_off + (size_t)g * ntr;
	const double2 *p0 = part + (size_t)e.part0 * npart + sc[lo].part_off + k;
	double2 st[8], ps[8];
#pragma unroll
	for (int m = 0; m < 8; m++) { st[m] = make_double2(0, 0); ps[m] = make_double2(0, 0); }
	for (unsigned b0 = 0; b0 < ntr; b0 += 4) { // four traces at a time: their loads are independent, the additions stay in trace order
		double2 a[4], u[4];
		double w[4][8]; // the traces' 8 weights, wave-uniform (the address depends on the block and the loop alone), loaded without a branch: the table ends with 3 spare blocks
#pragma unroll
		for (int j = 0; j < 4; j++) {
			a[j] = make_double2(0, 0);
			if (b0 + (unsigned)j < ntr) a[j] = p0[(size_t)(b0 + (unsigned)j) * npart];
#pragma unroll
			for (int m = 0; m < 8; m++) w[j][m] = readfirstlane_f64(wt[b0 + (unsigned)j].w[m]);
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
#pragma unroll
				for (int m = 0; m < 8; m++) {
					if (w[j][m] != 0.) { // a trace without weight takes no part: never 0 * Y
						st[m].x = fma(w[j][m], a[j].x, st[m].x); st[m].y = fma(w[j][m], a[j].y, st[m].y);
						ps[m].x = fma(w[j][m], u[j].x, ps[m].x); ps[m].y = fma(w[j][m], u[j].y, ps[m].y);
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

// time-domain linear stack of row q0 + blockIdx.y of ensemble blockIdx.z: the reference's FLOAT accumulator over the traces with weight in
// trace order (ts_pws1f_lib.c:538-542) with the addend w x -- acc = (float)((double)acc + w * (double)x), the product rounded on its own --
// then the float scale 1/W (:579-583); n+ = 0: a zero row.  w: the weight blocks as doubles.
__global__ void __launch_bounds__(256) k_wb_linear(const float *__restrict__ x, size_t ld, size_t N, const SbEns *__restrict__ ens,
                                                   const double *__restrict__ w, const unsigned *__restrict__ npos, const WbRow *__restrict__ rows, unsigned M,
                                                   unsigned q0, float *__restrict__ out)
{
#pragma clang fp contract(off) // w x is rounded before it is added
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const SbEns e = ens[blockIdx.z];
	const unsigned q = q0 + blockIdx.y;
	const size_t r = (size_t)blockIdx.z * M + q;
	float *o = out + ((size_t)e.row * M + q) * N;
	if (!npos[r]) { o[n] = 0.f; return; }
	const double *row = w + (e.bits_off + (size_t)(q >> 3) * e.m) * 8 + (q & 7u);
	const float *xe = x + (size_t)e.t0 * ld + n;
	const size_t mtr = e.m;
	float acc = 0.f;
	for (size_t i0 = 0; i0 < mtr; i0 += 8) { // eight rows' loads in flight (every row is loaded: no branch around a load); the additions keep the trace order
		float v[8];
		double c[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const size_t t = i0 + (size_t)j < mtr ? i0 + (size_t)j : mtr - 1;
			v[j] = xe[t * ld];
			c[j] = i0 + (size_t)j < mtr ? row[t * 8] : 0.; // (wave-uniform)
		}
#pragma unroll
		for (int j = 0; j < 8; j++)
			if (c[j] != 0.) acc = (float)((double)acc + c[j] * (double)v[j]);
	}
	o[n] = acc * (float)(1. / rows[r].W);
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

namespace {

struct Ens { unsigned b; size_t f, m; }; // ensemble with traces: index, first trace, traces

// the tables of a round in one block: ensembles | n+ of every row | (W, Keff) of every row | weight blocks + 3 spare ones (k_wb_accumulate loads
// the blocks of four traces at a time, whatever the ensemble's size)
struct WbTab { size_t ens, np, rows, w, bytes; };
WbTab wb_tab(size_t ne, size_t nrows, size_t nblocks)
{
	TableLayout lay;
	const size_t ens = lay.add<SbEns>(ne), np = lay.add<unsigned>(nrows), rows = lay.add<WbRow>(nrows), w = lay.add<Wb8>(nblocks + 3);
	return {ens, np, rows, w, lay.bytes};
}

// the ensembles E of the batch in rounds
int rounds_of(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t first0, const std::vector<Ens> &E, unsigned M, const double *h_w, size_t Tn,
              float *d_ls_out, float *d_ts_out, const unsigned *h_np, const WbRow *h_rows, BatchCall &call)
{
	const size_t N = pl->N, nc = pl->ncoef, n = E.size(), budget = tspws_part_budget_bytes();
	hipStream_t st = call.stream();
	const unsigned ng = (M + 7) / 8;
	int rc;
	void *v;
	// rounds of whole ensembles: the partials of their traces, a plane pair per (ensemble, row) and the tables (64 ng bytes a trace) within the
	// budget; ensembles within grid.z, partial indices and rows within 32 bits
	std::vector<size_t> tr0(n + 1, 0); // traces in front of ensemble j
	for (size_t j = 0; j < n; j++) tr0[j + 1] = tr0[j] + E[j].m;
	auto tab_of = [&](size_t j0, size_t j1) { return wb_tab(j1 - j0, (j1 - j0) * M, (tr0[j1] - tr0[j0]) * ng); };
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
	if (max_ntr > 0xfffffff0ull || max_ne * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "weighted_stack_batch: more than 2^32 traces or rows in one ensemble");
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
		pl->weighted_batch_stats.rounds++;
		const WbTab o = tab_of(r.j0, r.j1);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, "weighted_stack_batch: table bound"); // (cannot happen)
		char *blob = call.block(o.bytes), *tab;
		SbEns *he = (SbEns *)(blob + o.ens);
		unsigned *hnp = (unsigned *)(blob + o.np);
		WbRow *hrw = (WbRow *)(blob + o.rows);
		double *hw = (double *)(blob + o.w);
		size_t t = 0;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = E[j];
			SbEns d;
			d.t0 = e.f; d.bits_off = t * ng; d.m = (unsigned)e.m; d.part0 = (unsigned)t; d.row = e.b; d.pad = 0;
			he[j - r.j0] = d;
			memcpy(hnp + (j - r.j0) * (size_t)M, h_np + (size_t)e.b * M, (size_t)M * sizeof(unsigned));
			memcpy(hrw + (j - r.j0) * (size_t)M, h_rows + (size_t)e.b * M, (size_t)M * sizeof(WbRow));
			double *eb = hw + d.bits_off * 8; // (zero so far)
			for (unsigned q = 0; q < M; q++) {
				const double *row = h_w + (size_t)q * Tn + (e.f - first0);
				double *dst = eb + (size_t)(q >> 3) * e.m * 8 + (q & 7u);
				for (size_t i = 0; i < e.m; i++) dst[i * 8] = row[i];
			}
			t += e.m;
		}
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const SbEns *d_ens = (const SbEns *)(tab + o.ens);
		const unsigned *d_np = (const unsigned *)(tab + o.np);
		const WbRow *d_rows = (const WbRow *)(tab + o.rows);
		const Wb8 *d_w = (const Wb8 *)(tab + o.w);

		// every trace of the round once: a forward call per stretch of contiguous traces (empty ensembles in between do not cut a stretch)
		for (size_t j = r.j0; j < r.j1;) {
			size_t k = j + 1, nt = E[j].m;
			while (k < r.j1 && E[k].f == E[k - 1].f + E[k - 1].m) nt += E[k++].m;
			if ((rc = tspws_forward_parts<float>(pl, d_x + E[j].f * ld, nt, ld, part + (size_t)he[j - r.j0].part0 * pl->npart, st, nullptr, ScaleRange()))) return rc;
			j = k;
		}
		for (unsigned g0 = 0; g0 < ng; g0 += 65535)
			hipLaunchKernelGGL(k_wb_accumulate, dim3(pl->acc_blocks, std::min(65535u, ng - g0), (unsigned)ne), dim3(256), 0, st, (const double2 *)part, pl->npart,
			                   (const ScaleDesc *)pl->d_sc, pl->S, nc, d_ens, d_w, M, g0, planes);
		for (unsigned q0 = 0; q0 < M; q0 += 65535)
			hipLaunchKernelGGL(k_wb_linear, dim3(nb256, std::min(65535u, M - q0), (unsigned)ne), dim3(256), 0, st, d_x, ld, N, d_ens, (const double *)d_w, d_np, d_rows, M,
			                   q0, d_ls_out);
		// finish: the rows of the round in even batches
		for (size_t r0 = 0; r0 < nrows; r0 += RB) {
			const unsigned nr = (unsigned)std::min(RB, nrows - r0);
			hipLaunchKernelGGL(k_wb_weight, dim3((unsigned)((nc + 255) / 256), nr), dim3(256), 0, st, OUT, (const double2 *)planes, nc, d_np, d_rows, r0, p->wu, p->unbiased);
			if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nr, xr, (void *)st))) return rc;
			hipLaunchKernelGGL(k_sb_epilogue, dim3(nb256, nr), dim3(256), 0, st, (const double *)xr, N, d_ens, d_np, M, r0, d_ts_out);
		}
	}
	return 0;
}

} // namespace

extern "C" int tspws_hip_weighted_stack_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, unsigned M,
                                              const double *h_w, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, double *h_keff, void *s)
{
#pragma clang fp contract(off) // W, Q and Keff: every operation rounded on its own
	// what needs no plan comes first
	if (!p || !h_first) return fail(TSPWS_E_ARG, "weighted_stack_batch: NULL");
	if (!B || !M) return pl ? 0 : fail(TSPWS_E_ARG, "weighted_stack_batch: NULL");
	if (!h_w || !d_ls_out || !d_ts_out || !h_mtr_out) return fail(TSPWS_E_ARG, "weighted_stack_batch: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "weighted_stack_batch: decreasing ensemble offsets");
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m > 0xfffffff0ull) return fail(TSPWS_E_ARG, "weighted_stack_batch: more than 2^32 traces in an ensemble");
		if (m && tspws_is_two_stage(p, m))
			return fail(TSPWS_E_ARG, "weighted_stack_batch: a two-stage ensemble (0 < Kmax <= its traces): with real weights the groups of the two-stage stack have no meaning, only single-stage ensembles");
	}
	// n+, W, Keff of every row (refused before anything is written); the ensembles with traces
	const size_t Tn = h_first[B] - h_first[0], first0 = h_first[0];
	std::vector<Ens> E;
	std::vector<unsigned> np((size_t)B * M, 0);
	std::vector<WbRow> rows((size_t)B * M, WbRow{0, 0});
	for (unsigned b = 0; b < B; b++) {
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		for (unsigned q = 0; q < M; q++) {
			const double *row = h_w + (size_t)q * Tn + (f - first0);
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
	if (!pl) return fail(TSPWS_E_ARG, "weighted_stack_batch: NULL");
	if (Tn && !d_x) return fail(TSPWS_E_ARG, "weighted_stack_batch: NULL traces");
	if (Tn && ld < pl->N) return fail(TSPWS_E_ARG, "weighted_stack_batch: row stride below the trace length");
	const size_t N = pl->N;
	memcpy(h_mtr_out, np.data(), np.size() * sizeof(unsigned));
	if (h_keff) for (size_t r = 0; r < rows.size(); r++) h_keff[r] = rows[r].Keff;
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	int rc;
	tspws_hip_weighted_batch_stats &stats = pl->weighted_batch_stats;
	stats = tspws_hip_weighted_batch_stats();
	stats.shared = (unsigned)E.size();
	stats.empty = B - (unsigned)E.size();
	stats.rows = (unsigned)(E.size() * M);
	BatchCall call(st);
	if (!E.empty() && (rc = rounds_of(pl, p, d_x, ld, first0, E, M, h_w, Tn, d_ls_out, d_ts_out, np.data(), rows.data(), call))) return rc;
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
