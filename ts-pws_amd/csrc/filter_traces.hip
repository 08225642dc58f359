// filter_traces.hip -- the stack's coherence filter per trace (tspws_hip_filter_coef, tspws_hip_filter_traces): x~_i = ICWT(Y_i W), W the
// dimensionless weight that the stack applies to ST -- weight_value_eff without its ST and 1 / M factors -- made from the phase stack PS of
// the whole ensemble (Baig et al. 2009, Hadziioannou et al. 2011 with the S transform).  By linearity the mean of an ensemble's filtered
// traces is its tsPWS row.  Leave-one-out: trace i is filtered with the W of PS - u_i and K - 1, u_i the unit phasor that the accumulation
// added for it.  Targets are the ensembles' own traces or M rows per ensemble ([B][M][ldr] floats with [B][M] host counts, what the batched
// calls leave).
//
//   host         filter_plan.h: what a row and an ensemble cost, the rounds of whole ensembles, the chunks of an ensemble that exceeds the
//                budget alone, the slabs (up to 8 consecutive participating rows of one ensemble), ONE table block and one upload per pass.
//                A round: ONE tspws_hip_forward_f32 on its targets; PS per ensemble from the existing calls (tspws_hip_accumulate on the sets
//                just made, tspws_hip_stacks_float on the ensemble's traces, or tspws_hip_partial_stacks + tspws_hip_stacks_double: the
//                phasor rule has its one copy there); the kernels below; tspws_hip_inverse (ONE call, unless its octave buffer for the whole
//                round would exceed the budget); the cast.
//   k_cf_weight  one thread per (ensemble of the pass, coefficient): W from PS, 8 B per coefficient -- pow and hypot once per ensemble
//   k_cf_apply   (tile of 256 coefficients) x (slab): a thread holds W (leave-one-out: PS, K - 1 and the mode) in registers, issues the
//                slab's 16-byte loads of Y before the first multiply and stores Y W with 16-byte stores; under leave-one-out it forms u_i
//                from the stored Y_i through add_unit_phasor on a zero accumulator and W_i per row
//   k_cf_rows    the inverse's FP64 rows as floats at the output's row stride; NaN for the rows left out
// No LDS, nothing atomic, every output has one writer; every product and sum of W and Y W is rounded on its own.  A row's output depends
// on its own set, its ensemble's PS and count and the mode alone: a repeated call is bit-identical, and the rounds, chunks and slabs change
// no bit of filter_coef's outputs.
#include "tspws_internal.h"
#include "coef_rows.h"
#include "filter_plan.h"

static_assert(sizeof(CfSlab) == 12 && sizeof(CfEns) == 16 && CF_SLAB == 8, "the tables' layout");

// the weight of one coefficient: weight_value_eff's operations in its order, without the factors ST and 1 / M
__device__ __forceinline__ double cf_weight(const double2 ps, const int mode, const double K, const double wu)
{
#pragma clang fp contract(off)
	if (mode == 0) {
		const double g = 1. / (K * K);
		return (ps.x * ps.x + ps.y * ps.y) * g;
	} else if (mode == 1) {
		const double g = 1. / K;
		return hypot(ps.x, ps.y) * g;
	} else if (mode == 2) {
		return pow(hypot(ps.x, ps.y) / K, wu);
	}
	const double iK = 1. / K, iK1 = 1. / (K - 1);
	const double px = ps.x * iK, py = ps.y * iK;
	const double c = px * px + py * py;
	return (K * c - 1) * iK1;
}

__global__ void __launch_bounds__(256) k_cf_weight(const double2 *__restrict__ PS, size_t ncoef, const CfEns *__restrict__ ens, double wu, double *__restrict__ W)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= ncoef) return;
	const CfEns en = ens[blockIdx.y];
	const size_t o = (size_t)blockIdx.y * ncoef + i;
	W[o] = cf_weight(PS[o], en.mode, en.K, wu);
}

// block = slab * ntiles + tile.  Y and out may be the same sets (in place): a thread reads and writes its own coefficients only.
template <bool LOO>
__global__ void __launch_bounds__(256) k_cf_apply(const double2 *Y, size_t ncoef, unsigned ntiles, const CfSlab *__restrict__ slabs, const CfEns *__restrict__ ens,
                                                  const double2 *__restrict__ PS, const double *__restrict__ W, double wu, double2 *out)
{
#pragma clang fp contract(off)
	const CfSlab sl = slabs[blockIdx.x / ntiles];
	const size_t i = (size_t)(blockIdx.x % ntiles) * 256 + threadIdx.x;
	if (i >= ncoef) return;
	const size_t at = (size_t)sl.row0 * ncoef + i, pe = (size_t)sl.ens * ncoef + i;
	double2 y[CF_SLAB];
#pragma unroll
	for (unsigned r = 0; r < CF_SLAB; r++)
		if (r < sl.n) y[r] = Y[at + (size_t)r * ncoef];
	if (!LOO) {
		const double w = W[pe];
#pragma unroll
		for (unsigned r = 0; r < CF_SLAB; r++)
			if (r < sl.n) out[at + (size_t)r * ncoef] = make_double2(y[r].x * w, y[r].y * w);
	} else {
		const double2 ps = PS[pe];
		const CfEns en = ens[sl.ens];
#pragma unroll
		for (unsigned r = 0; r < CF_SLAB; r++)
			if (r < sl.n) {
				double2 u = make_double2(0.0, 0.0);
				add_unit_phasor(u, y[r]); // what the accumulation added for this trace: nothing when the rule skipped it
				const double w = cf_weight(make_double2(ps.x - u.x, ps.y - u.y), en.mode, en.K, wu);
				out[at + (size_t)r * ncoef] = make_double2(y[r].x * w, y[r].y * w);
			}
	}
}

// block = row * nbx + column block
__global__ void __launch_bounds__(256) k_cf_rows(const double *__restrict__ x, unsigned N, unsigned nbx, const unsigned *__restrict__ live, float *__restrict__ out, size_t ldo)
{
	const size_t row = blockIdx.x / nbx;
	const unsigned n = (blockIdx.x % nbx) * 256 + threadIdx.x;
	if (n >= N) return;
	out[row * ldo + n] = live[row] ? (float)x[row * N + n] : __int_as_float(0x7fc00000);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
namespace {

struct CfPass { const unsigned *d_live = nullptr; };

// The weights of one pass applied: the sets Y of n rows -> out (Y itself: in place); ens[i] = the row's ensemble among the pass's nens, or
// NOSLOT; PS / W: the ensembles' planes (W is written here when make_w says so; unused under leave-one-out).  The table slot is reserved for
// passes of max_rows rows and max_ens ensembles.
int cf_apply_pass(tspws_hip_plan *pl, BatchCall &call, const char *who, const double2 *Y, double2 *out, const unsigned *ens, size_t n, const CfEns *en, size_t nens,
                  const double2 *PS, double *W, double wu, int loo, bool make_w, size_t max_rows, size_t max_ens, CfPass *ps)
{
	hipStream_t st = call.stream();
	const std::vector<CfSlab> slabs = cf_slabs(ens, n);
	const CfTab o = cf_tab(slabs.size(), nens, n);
	const unsigned ntiles = (unsigned)((pl->ncoef + 255) / 256);
	if ((unsigned long long)slabs.size() * ntiles > 0x7fffffffull || nens > 65535)
		return fail(TSPWS_E_ARG, (std::string(who) + ": more than 2^31 workgroups or 65535 ensembles in a pass").c_str());
	char *blob = call.block(o.bytes), *tab;
	cf_fill(blob, o, slabs, en, nens, ens, n);
	if (int rc = call.upload(pl, SCR_CFTAB, blob, o.bytes, &tab, cf_tab(max_rows, max_ens, max_rows).bytes)) return rc;
	const CfEns *d_en = (const CfEns *)(tab + o.ens);
	if (!loo && make_w && nens) hipLaunchKernelGGL(k_cf_weight, dim3(ntiles, (unsigned)nens), dim3(256), 0, st, PS, pl->ncoef, d_en, wu, W);
	if (!slabs.empty()) {
		const dim3 grid((unsigned)(slabs.size() * ntiles));
		if (loo) hipLaunchKernelGGL(k_cf_apply<true>, grid, dim3(256), 0, st, Y, pl->ncoef, ntiles, (const CfSlab *)(tab + o.slabs), d_en, PS, (const double *)W, wu, out);
		else hipLaunchKernelGGL(k_cf_apply<false>, grid, dim3(256), 0, st, Y, pl->ncoef, ntiles, (const CfSlab *)(tab + o.slabs), d_en, PS, (const double *)W, wu, out);
	}
	if (ps) ps->d_live = (const unsigned *)(tab + o.live);
	return 0;
}

// the count and mode in force for an ensemble of K stacked units
CfEns cf_ens(double wu, int unbiased, unsigned K, int loo)
{
	const unsigned Ke = loo ? K - 1 : K;
	return {(double)Ke, tspws_weight_mode(wu, unbiased, Ke), 0u};
}

} // namespace

extern "C" int tspws_hip_filter_coef(tspws_hip_plan *pl, const double *d_Y, const unsigned *h_ens, size_t nrow, const double *d_PS, const unsigned *h_K, unsigned B,
                                     double wu, int unbiased, int loo, double *d_out, void *s)
{
	const char *who = "filter_coef";
	if (!d_Y || !d_PS || !h_K) return fail(TSPWS_E_ARG, "filter_coef: NULL");
	if (loo != 0 && loo != 1) return fail(TSPWS_E_ARG, "filter_coef: loo must be 0 or 1");
	if (!std::isfinite(wu)) return fail(TSPWS_E_ARG, "filter_coef: a NaN or infinite power");
	if (nrow > 0xfffffff0ull) return fail(TSPWS_E_ARG, "filter_coef: more than 2^32 - 16 rows");
	for (unsigned b = 0; b < B; b++)
		if (h_K[b] < (loo ? 2u : 1u)) return fail(TSPWS_E_ARG, loo ? "filter_coef: leave-one-out needs counts >= 2" : "filter_coef: a count of 0");
	if (!pl) return fail(TSPWS_E_ARG, "filter_coef: NULL");
	if (!nrow || !B) return 0;
	if (!h_ens && nrow != B) return fail(TSPWS_E_ARG, "filter_coef: without h_ens the rows must number B");
	if (h_ens)
		for (size_t i = 0; i < nrow; i++)
			if (h_ens[i] >= B) return fail(TSPWS_E_ARG, "filter_coef: an ensemble index >= B");
	if (B > 65535) return fail(TSPWS_E_ARG, "filter_coef: more than 65535 ensembles");

	HIP_TRY(hipSetDevice(pl->device));
	std::vector<CfEns> en(B);
	for (unsigned b = 0; b < B; b++) en[b] = cf_ens(wu, unbiased, h_K[b], loo);
	void *v = nullptr;
	if (!loo)
		if (int rc = scratch(pl, SCR_CFP, (size_t)B * pl->ncoef * sizeof(double), &v)) return rc;
	const size_t chunk = std::min<size_t>(nrow, 32768);
	BatchCall call(S_(s));
	pl->filter_stats = tspws_hip_filter_stats();
	return coef_chunks(call, row_counters(pl->filter_stats), (const double2 *)d_Y, nullptr, pl->ncoef, h_ens, nrow, chunk,
	                   [&](const double2 *Y, const double2 *, const unsigned *ens, size_t n, size_t row0, size_t max_rows) {
		                   double2 *out = d_out ? (double2 *)d_out + row0 * pl->ncoef : const_cast<double2 *>(Y);
		                   return cf_apply_pass(pl, call, who, Y, out, ens, n, en.data(), B, (const double2 *)d_PS, (double *)v, wu, loo, row0 == 0, max_rows, B, nullptr);
	                   });
}

extern "C" int tspws_hip_filter_traces(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, const float *d_rows,
                                       size_t ldr, unsigned M, const unsigned *h_mtr, int loo, float *d_out, size_t ldo, void *s)
{
	const char *who = "filter_traces";
	// what needs no plan
	if (!p || !h_first || !d_out) return fail(TSPWS_E_ARG, "filter_traces: NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "filter_traces: decreasing ensemble offsets");
	if (loo != 0 && loo != 1) return fail(TSPWS_E_ARG, "filter_traces: loo must be 0 or 1");
	if (d_rows && !M) return fail(TSPWS_E_ARG, "filter_traces: target rows without M");
	if (!d_rows && (M || h_mtr)) return fail(TSPWS_E_ARG, "filter_traces: M or counts without target rows");
	if (loo && d_rows) return fail(TSPWS_E_ARG, "filter_traces: leave-one-out takes the ensembles' own traces, not target rows");
	bool any2 = false;
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m && tspws_is_two_stage(p, m)) any2 = true;
	}
	if (loo && any2) return fail(TSPWS_E_ARG, "filter_traces: leave-one-out with a two-stage ensemble");
	const size_t T = B ? h_first[B] - h_first[0] : 0;
	if (T && !d_x) return fail(TSPWS_E_ARG, "filter_traces: NULL");
	if ((d_rows ? (unsigned long long)B * M : (unsigned long long)T) > 0xfffffff0ull) return fail(TSPWS_E_ARG, "filter_traces: more than 2^32 - 16 rows");
	if (!pl) return fail(TSPWS_E_ARG, "filter_traces: NULL");
	const size_t N = pl->N, nc = pl->ncoef;
	if ((T && ld < N) || (d_rows && ldr < N) || ldo < N) return fail(TSPWS_E_ARG, "filter_traces: row stride below the trace length");
	if (!B) return 0;

	const double wu = p->wu;
	const unsigned Kmax = p->Kmax;
	std::vector<size_t> rows0(B + 1);
	for (unsigned b = 0; b <= B; b++) rows0[b] = d_rows ? (size_t)b * M : h_first[b] - h_first[0];
	const size_t budget = tspws_part_budget_bytes();
	const CfCost cost = cf_cost(nc, N, any2 ? Kmax : 0);
	const std::vector<Round> rounds = cf_rounds(rows0.data(), B, cost, budget);
	size_t max_rows = 1, max_ens = 1;
	for (const Round &r : rounds) {
		const size_t n = rows0[r.j1] - rows0[r.j0];
		max_rows = std::max(max_rows, cf_round_fits(rows0.data(), r, cost, budget) ? n : cf_chunk_rows(n, cost, budget));
		max_ens = std::max(max_ens, r.j1 - r.j0);
	}
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_CFY, max_rows * nc * sizeof(double2), &v))) return rc;
	double2 *Y = (double2 *)v;
	if ((rc = scratch(pl, SCR_CFX, max_rows * N * sizeof(double), &v))) return rc;
	double *X = (double *)v;
	if ((rc = scratch(pl, SCR_CFP, (1 + max_ens) * nc * sizeof(double2) + max_ens * nc * sizeof(double), &v))) return rc;
	double2 *ST = (double2 *)v, *PS = ST + nc;
	double *W = (double *)(PS + max_ens * nc);
	double *R = nullptr;
	if (any2) {
		if ((rc = scratch(pl, SCR_CFR, (size_t)Kmax * N * sizeof(double), &v))) return rc;
		R = (double *)v;
	}
	BatchCall call(st);
	tspws_hip_filter_stats &stats = pl->filter_stats;
	stats = tspws_hip_filter_stats();

	// PS of ensemble b into PSe: from its sets (single-stage, the targets are its traces and their sets are at hand) or from its traces
	auto make_ps = [&](unsigned b, const double2 *sets, double2 *PSe) -> int {
		const size_t m = h_first[b + 1] - h_first[b];
		const float *x = d_x + h_first[b] * ld;
		if (!m) return 0;
		if (tspws_is_two_stage(p, m)) {
			if (int e = tspws_hip_partial_stacks(pl, x, ld, m, 0, m, Kmax, R, N, s)) return e;
			return tspws_hip_stacks_double(pl, R, Kmax, N, (double *)ST, (double *)PSe, s);
		}
		if (sets) return tspws_hip_accumulate(pl, (const double *)sets, m, (double *)ST, (double *)PSe, 1, s);
		return tspws_hip_stacks_float(pl, x, m, ld, (double *)ST, (double *)PSe, s);
	};
	// forward transform of the target rows [r0, r0 + n) into Y
	auto forward = [&](size_t r0, size_t n) -> int {
		return d_rows ? tspws_hip_forward_f32(pl, d_rows + r0 * ldr, n, ldr, (double *)Y, s)
		              : tspws_hip_forward_f32(pl, d_x + (h_first[0] + r0) * ld, n, ld, (double *)Y, s);
	};
	// weights, inverse and cast of the sets in Y: the target rows [r0, r0 + n)
	auto finish = [&](size_t r0, size_t n, const unsigned *ens, const CfEns *en, size_t nens, bool make_w) -> int {
		CfPass ps;
		if (int e = cf_apply_pass(pl, call, who, Y, Y, ens, n, en, nens, PS, W, wu, loo, make_w, max_rows, max_ens, &ps)) return e;
		// ONE inverse call, unless its octave buffer would exceed the budget
		const size_t ni = cf_inverse_rows(n, tspws_inverse_row_bytes(pl), budget);
		for (size_t i0 = 0; i0 < n; i0 += ni)
			if (int e = tspws_hip_inverse(pl, (const double *)(Y + i0 * nc), std::min(ni, n - i0), X + i0 * N, s)) return e;
		const unsigned nbx = (unsigned)((N + 255) / 256);
		if ((unsigned long long)n * nbx > 0x7fffffffull) return fail(TSPWS_E_ARG, "filter_traces: more than 2^31 workgroups in a pass");
		hipLaunchKernelGGL(k_cf_rows, dim3((unsigned)(n * nbx)), dim3(256), 0, st, (const double *)X, (unsigned)N, nbx, ps.d_live, d_out + r0 * ldo, ldo);
		return 0;
	};

	std::vector<unsigned> ens;
	std::vector<CfEns> en;
	for (const Round &r : rounds) {
		const size_t r0 = rows0[r.j0], n = rows0[r.j1] - r0, nens = r.j1 - r.j0;
		ens.assign(n, NOSLOT);
		en.assign(nens, CfEns{1.0, 0, 0u});
		for (size_t b = r.j0; b < r.j1; b++) {
			const size_t m = h_first[b + 1] - h_first[b];
			const bool two = m && tspws_is_two_stage(p, m);
			if (!m) stats.empty++; else if (two) stats.two_stage++; else stats.single_stage++;
			const bool out = !m || (loo && m < 2); // no weight to filter with
			if (!out) en[b - r.j0] = cf_ens(wu, p->unbiased, two ? Kmax : (unsigned)m, loo);
			for (size_t i = rows0[b]; i < rows0[b + 1]; i++) {
				const bool in = !out && (!d_rows || !h_mtr || h_mtr[i] > 0);
				if (in) ens[i - r0] = (unsigned)(b - r.j0);
				stats.rows += in;
				stats.left_out += !in;
			}
		}
		stats.rounds++;
		if (!n) continue;
		if (cf_round_fits(rows0.data(), r, cost, budget)) {
			if ((rc = forward(r0, n))) return rc;
			for (size_t b = r.j0; b < r.j1; b++)
				if ((rc = make_ps((unsigned)b, d_rows ? nullptr : Y + (rows0[b] - r0) * nc, PS + (b - r.j0) * nc))) return rc;
			if ((rc = finish(r0, n, ens.data(), en.data(), nens, true))) return rc;
			continue;
		}
		// one ensemble whose sets alone exceed the budget: its PS first, chunk by chunk, then its targets again in chunks
		const unsigned b = (unsigned)r.j0;
		const size_t m = h_first[b + 1] - h_first[b], chunk = cf_chunk_rows(n, cost, budget);
		if (!d_rows && m && !tspws_is_two_stage(p, m)) {
			stats.twice++;
			for (size_t c0 = 0; c0 < n; c0 += chunk) {
				const size_t k = std::min(chunk, n - c0);
				if ((rc = forward(r0 + c0, k))) return rc;
				if ((rc = tspws_hip_accumulate(pl, (const double *)Y, k, (double *)ST, (double *)PS, c0 == 0, s))) return rc;
			}
		} else if ((rc = make_ps(b, nullptr, PS))) return rc;
		for (size_t c0 = 0; c0 < n; c0 += chunk) {
			const size_t k = std::min(chunk, n - c0);
			if ((rc = forward(r0 + c0, k))) return rc;
			if ((rc = finish(r0 + c0, k, ens.data() + c0, en.data(), 1, c0 == 0))) return rc;
		}
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_filter_traces_stats(const tspws_hip_plan *pl, tspws_hip_filter_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "filter_traces_stats: NULL");
	*stats = pl->filter_stats;
	return 0;
}
