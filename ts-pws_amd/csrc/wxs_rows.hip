// wxs_rows.hip -- dv/v per band from the wavelet cross-spectrum (tspws_hip_wxs_coef, tspws_hip_wxs_rows): per (row, window, band) nine sums
// over the coefficients of the row's set Yc against its reference's set Yr -- the cross-spectrum X = c conj(r), its modulus a, the delay
// delta = arg X / omega_s and the lag t = k D_s - z -- and from them the weighted regression of the delay on the lag.  Rows are what the
// batched calls write ([B][M][ld] floats, [B][M] host counts); tspws_hip_wxs_rows transforms them in rounds with tspws_hip_forward_f32.
//
//   host         wxs_plan.h: the scales in use, the index range of every (scale, window) after the wrap rule, the items (segments of WX_SEG
//                coefficients of one scale and window) that all rows share, the tasks (runs of short items), the rounds, ONE table block and
//                one upload per pass
//   k_wx_reduce  one WAVE per (participating row, task): item after item, the lanes read consecutive complex coefficients of Yc and Yr
//                (16 B per lane, 1 KB per wave and load; the next pass's loads are in flight while a pass computes), every lane keeps the nine
//                sums of its coefficients (in increasing k) in FP64 registers, the wave adds them in the fixed lane order of valu_reduce16
//                (lane_reduce.h) and leaves one 72-byte partial per item.  Each set is read once per window that covers it.
//   k_wx_final   one thread per (row, window, band): adds the partials of the band's scales in increasing s, of each scale's segments in
//                increasing order, and forms the fit; NaN and -1 for the rows left out
// Nothing is atomic, every output has one writer, and the order of every sum depends on the scale, the window, the wrap rule and the band's
// range alone: a repeated call is bit-identical, and nrow, B, M, the other bands and windows, the rounds and the padding change no bit.
#include "tspws_internal.h"
#include "coef_rows.h"
#include "lane_reduce.h"

static_assert(sizeof(WxBand) == sizeof(tspws_band) && sizeof(WxItem) == 32 && WX_SEG == 4 * 64, "the tables' layout");

// part[(slot nitems + item) WX_NSUM + e] for the items of the wave's task
__global__ void __launch_bounds__(256) k_wx_reduce(const double2 *__restrict__ Yc, const double2 *__restrict__ Yr, size_t ncoef, const WxItem *__restrict__ items,
                                                   unsigned nitems, const WxTask *__restrict__ tasks, unsigned ntasks, const WxRow *__restrict__ list, double z,
                                                   unsigned long long nwork, double *__restrict__ part)
{
#pragma clang fp contract(off) // every operation of the definition is rounded on its own
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long work = (unsigned long long)blockIdx.x * 4 + wave;
	if (work >= nwork) return; // (the whole wave)
	const unsigned task = (unsigned)(work % ntasks);
	const size_t slot = (size_t)(work / ntasks);
	const WxRow rw = list[slot];
	const double2 *__restrict__ yc = Yc + (size_t)rw.row * ncoef;
	const double2 *__restrict__ yr = Yr + (size_t)rw.ens * ncoef;
	const WxTask tk = tasks[task];
	// the lane that holds element e of valu_reduce16's result: bits 5, 4, 3, 2 of the lane = bits 3, 2, 1, 0 of e (the first lane of the quad writes)
	const unsigned mine = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
	for (unsigned i = tk.first; i < tk.first + tk.n; i++) {
		const WxItem it = items[i];
		double v[16];
#pragma unroll
		for (int e = 0; e < 16; e++) v[e] = 0.0;
		// pass p: coefficient lane + 64 p of the item; the next pass's loads are in flight while this one computes
		const size_t at0 = it.coef + (lane < it.count ? lane : 0u); // (an item holds at least one coefficient)
		double2 c = yc[at0], r = yr[at0];
		const unsigned npass = (it.count + 63) / 64; // (wave-uniform)
#pragma unroll 1
		for (unsigned p = 0; p < npass; p++) {
			const unsigned j = lane + 64 * p, jn = j + 64;
			const size_t atn = it.coef + (jn < it.count ? jn : 0u);
			const double2 cn = yc[atn], rn = yr[atn];
			const double xr = c.x * r.x + c.y * r.y, xi = c.y * r.x - c.x * r.y;
			const double a = hypot(xr, xi);
			if (j < it.count && a > 0.0 && a < __longlong_as_double(0x7ff0000000000000ll)) {
				const double delta = atan2(xi, xr) / it.omega;
				const double t = (double)((unsigned long long)(it.k0 + j) * it.D) - z;
				const double at = a * t, ad = a * delta;
				v[0] += 1.0;
				v[1] += a;
				v[2] += at;
				v[3] += at * t;
				v[4] += ad;
				v[5] += at * delta;
				v[6] += ad * delta;
				v[7] += xr;
				v[8] += xi;
			}
			c = cn; r = rn;
		}
		const double sum = valu_reduce16(v, lane);
		if ((lane & 3) == 0 && mine < WX_NSUM) part[(slot * nitems + i) * WX_NSUM + mine] = sum;
	}
}

// hypot of two finite doubles with one correction step (Borges, "An improved algorithm for hypot(a, b)", the fused and corrected form) on
// operands scaled by an exact power of two: the correctly rounded value in all but rare cases
__device__ __forceinline__ double wx_hypot(double x, double y)
{
#pragma clang fp contract(off) // (only the fma calls below are fused)
	x = fabs(x); y = fabs(y);
	if (x < y) { const double s = x; x = y; y = s; }
	if (!(x > 0.0) || !(x < __longlong_as_double(0x7ff0000000000000ll))) return x + y; // 0, Inf or NaN
	const int e = ilogb(x);
	x = ldexp(x, -e); y = ldexp(y, -e);
	double h = sqrt(fma(x, x, y * y));
	const double h2 = h * h, x2 = x * x;
	const double d = (fma(-y, y, h2 - x2) + fma(h, h, -h2)) - fma(x, x, -x2);
	h = h - d / (2.0 * h);
	return ldexp(h, e);
}

// sums[(row0 + row) W + w) R + band][WX_NSUM] (when given) and fit[..][WX_NFIT] of every (row, window, band) of the pass
__global__ void __launch_bounds__(256) k_wx_final(const double *__restrict__ part, unsigned nitems, const WxSpan *__restrict__ spans, const unsigned *__restrict__ uidx,
                                                  const WxBand *__restrict__ bands, unsigned R, unsigned W, const unsigned *__restrict__ slot_of, size_t row0,
                                                  unsigned long long nout, double *__restrict__ sums, double *__restrict__ fit)
{
#pragma clang fp contract(off)
	const unsigned long long o = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (o >= nout) return;
	const unsigned band = (unsigned)(o % R), w = (unsigned)((o / R) % W);
	const size_t row = (size_t)(o / R / W);
	const size_t out = (size_t)row0 * W * R + o;
	const unsigned slot = slot_of[row];
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	double *__restrict__ fo = fit + out * WX_NFIT;
	if (slot == NOSLOT) { // the row does not take part
		if (sums)
			for (int e = 0; e < WX_NSUM; e++) sums[out * WX_NSUM + e] = nan;
		for (int e = 0; e < 5; e++) fo[e] = nan;
		fo[5] = -1.0;
		return;
	}
	double s[WX_NSUM];
#pragma unroll
	for (int e = 0; e < WX_NSUM; e++) s[e] = 0.0;
	const WxBand b = bands[band];
	for (unsigned sc = b.s_begin; sc < b.s_end; sc++) {
		const WxSpan sp = spans[(size_t)uidx[sc] * W + w];
		const double *__restrict__ p = part + ((size_t)slot * nitems + sp.first) * WX_NSUM;
		for (unsigned i = 0; i < sp.n; i++)
#pragma unroll
			for (int e = 0; e < WX_NSUM; e++) s[e] += p[(size_t)i * WX_NSUM + e];
	}
	if (sums)
#pragma unroll
		for (int e = 0; e < WX_NSUM; e++) sums[out * WX_NSUM + e] = s[e];
	const double n = s[0], A = s[1], At = s[2], Att = s[3], Ad = s[4], Atd = s[5], Add = s[6];
	const double coh = wx_hypot(s[7], s[8]) / A; // (A == 0: 0 / 0)
	const double den = A * Att - At * At;
	double eh = nan, ic = nan, err = nan, rms = nan;
	if (n >= 2.0 && den > 0.0) {
		eh = (A * Atd - At * Ad) / den;
		ic = (Att * Ad - At * Atd) / den;
		const double res = (Add - ic * Ad) - eh * Atd;
		rms = sqrt((res > 0.0 ? res : 0.0) / A);
		err = rms * sqrt(A / den);
	}
	fo[0] = eh; fo[1] = ic; fo[2] = err; fo[3] = rms; fo[4] = coh; fo[5] = n;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the checks both entry points share, in the contract's order: first what needs no plan (pl may be NULL there)
static int wx_check_tables(const tspws_hip_plan *pl, const char *who, double z, const tspws_band *bands, unsigned R, const size_t *win, unsigned W)
{
	const std::string w(who);
	if (!pl) {
		if (!R || R > WX_RMAX) return fail(TSPWS_E_ARG, (w + ": 1 to 64 bands").c_str());
		if (const char *e = range_count_error(W, WINDOWS)) return refuse(who, e);
		if (int rc = tspws_bands_check(nullptr, bands, R, who)) return rc;
		if (const char *e = range_empty_error(win, W, WINDOWS)) return refuse(who, e);
		if (!std::isfinite(z)) return fail(TSPWS_E_ARG, (w + ": a NaN or infinite zero-lag position").c_str());
		return 0;
	}
	if (int rc = tspws_bands_check(pl, bands, R, who)) return rc;
	if (const char *e = range_past_error(win, W, pl->N, WINDOWS)) return refuse(who, e);
	return 0;
}

static WxPlan wx_plan_of(const tspws_hip_plan *pl, const tspws_band *bands, unsigned R, const size_t *win, unsigned W, int skip_wrapped)
{
	std::vector<WxScale> sc = wx_scales_of(pl);
	for (unsigned s = 0; s < pl->S; s++) sc[s].omega = pl->w0 / pl->sc[s].scale; // (rad per sample: tspws_bands_from_frequencies' centre frequency times 2 pi dt)
	return wx_plan(sc.data(), pl->S, pl->N, (const WxBand *)bands, R, win, W, skip_wrapped);
}

// one pass: the rows [0, nrows) of Yc against the sets ens[.] of Yr (NOSLOT: the row does not take part); outputs from row `row0` on; the
// slots are reserved for a pass of max_rows rows
static int wx_pass(tspws_hip_plan *pl, BatchCall &call, const char *who, const WxPlan &P, const tspws_band *bands, unsigned R, const double2 *Yc,
                   const double2 *Yr, const unsigned *ens, size_t nrows, size_t row0, double z, size_t max_rows, double *d_sums, double *d_fit)
{
	hipStream_t st = call.stream();
	const size_t nslots = count_slots(ens, nrows), max_tab = wx_tab(P, R, max_rows, max_rows).bytes, max_part = wx_part_bytes(P, max_rows);
	const WxTab o = wx_tab(P, R, nslots, nrows);
	const unsigned nitems = (unsigned)P.items.size(), ntasks = (unsigned)P.tasks.size();
	const unsigned long long nwork = (unsigned long long)nslots * ntasks, nout = (unsigned long long)nrows * P.W * R;
	if ((nwork + 3) / 4 > 0x7fffffffull || (nout + 255) / 256 > 0x7fffffffull) return fail(TSPWS_E_ARG, (std::string(who) + ": more than 2^33 waves in a round").c_str());
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_WXP, std::max<size_t>({wx_part_bytes(P, nslots), max_part, 16}), &v))) return rc;
	double *part = (double *)v;
	char *blob = call.block(o.bytes), *tab;
	wx_fill(blob, o, P, (const WxBand *)bands, R, ens, nrows);
	if ((rc = call.upload(pl, SCR_WXTAB, blob, o.bytes, &tab, max_tab))) return rc;
	if (nwork)
		hipLaunchKernelGGL(k_wx_reduce, dim3((unsigned)((nwork + 3) / 4)), dim3(256), 0, st, Yc, Yr, pl->ncoef, (const WxItem *)(tab + o.items), nitems,
		                   (const WxTask *)(tab + o.tasks), ntasks, (const WxRow *)(tab + o.list), z, nwork, part);
	hipLaunchKernelGGL(k_wx_final, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, (const double *)part, nitems, (const WxSpan *)(tab + o.spans),
	                   (const unsigned *)(tab + o.uidx), (const WxBand *)(tab + o.bands), R, P.W, (const unsigned *)(tab + o.slot_of), row0, nout, d_sums, d_fit);
	return 0;
}

static void wx_stats_begin(tspws_hip_plan *pl, const WxPlan &P)
{
	pl->wxs_stats = tspws_hip_wxs_stats();
	pl->wxs_stats.items = (unsigned)P.items.size();
	pl->wxs_stats.scales = (unsigned)P.used.size();
}

extern "C" int tspws_hip_wxs_coef(tspws_hip_plan *pl, const double *d_Yc, const double *d_Yr, const unsigned *h_ens, size_t nrow, unsigned B, double z,
                                  const tspws_band *h_bands, unsigned R, const size_t *h_win, unsigned W, int skip_wrapped, double *d_sums, double *d_fit, void *s)
{
	const char *who = "wxs_coef";
	if (!d_Yc || !d_Yr || !h_bands || !h_win || !d_fit) return fail(TSPWS_E_ARG, "wxs_coef: NULL");
	if (int rc = wx_check_tables(nullptr, who, z, h_bands, R, h_win, W)) return rc;
	if (!pl) return fail(TSPWS_E_ARG, "wxs_coef: NULL");
	if (int rc = wx_check_tables(pl, who, z, h_bands, R, h_win, W)) return rc;
	if (!nrow || !B) return 0;
	if (!h_ens && nrow != B) return fail(TSPWS_E_ARG, "wxs_coef: without h_ens the rows must number B");
	if (h_ens)
		for (size_t i = 0; i < nrow; i++)
			if (h_ens[i] >= B) return fail(TSPWS_E_ARG, "wxs_coef: an ensemble index >= B");
	if (nrow > 0xfffffff0ull) return fail(TSPWS_E_ARG, "wxs_coef: more than 2^32 - 16 rows");

	const WxPlan P = wx_plan_of(pl, h_bands, R, h_win, W, skip_wrapped);
	const size_t chunk = wx_chunk_rows(nrow, P, R, tspws_part_budget_bytes());
	HIP_TRY(hipSetDevice(pl->device));
	BatchCall call(S_(s));
	wx_stats_begin(pl, P);
	return coef_chunks(call, row_counters(pl->wxs_stats), (const double2 *)d_Yc, (const double2 *)d_Yr, pl->ncoef, h_ens, nrow, chunk,
	                   [&](const double2 *Yc, const double2 *Yr, const unsigned *ens, size_t n, size_t row0, size_t max_rows) {
		                   return wx_pass(pl, call, who, P, h_bands, R, Yc, Yr, ens, n, row0, z, max_rows, d_sums, d_fit);
	                   });
}

extern "C" int tspws_hip_wxs_rows(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                                  size_t ldr, double z, const tspws_band *h_bands, unsigned R, const size_t *h_win, unsigned W, int skip_wrapped, double *d_sums,
                                  double *d_fit, void *s)
{
	const char *who = "wxs_rows";
	if (!d_rows || !d_ref || !h_bands || !h_win || !d_fit) return fail(TSPWS_E_ARG, "wxs_rows: NULL");
	if (int rc = wx_check_tables(nullptr, who, z, h_bands, R, h_win, W)) return rc;
	if (!pl) return fail(TSPWS_E_ARG, "wxs_rows: NULL");
	if (ld < pl->N) return fail(TSPWS_E_ARG, "wxs_rows: row stride below the trace length");
	if (ldr < pl->N) return fail(TSPWS_E_ARG, "wxs_rows: reference row stride below the trace length");
	if (int rc = wx_check_tables(pl, who, z, h_bands, R, h_win, W)) return rc;
	if (!B || !M) return 0;
	if ((unsigned long long)B * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "wxs_rows: more than 2^32 - 16 rows");

	const WxPlan P = wx_plan_of(pl, h_bands, R, h_win, W, skip_wrapped);
	const std::vector<Round> rounds = wx_rounds(B, M, pl->ncoef, P, R, tspws_part_budget_bytes());
	HIP_TRY(hipSetDevice(pl->device));
	BatchCall call(S_(s));
	wx_stats_begin(pl, P);
	return coef_rounds(pl, call, row_counters(pl->wxs_stats), d_rows, ld, M, h_mtr, d_ref, ldr, 1, rounds, SCR_WXY,
	                   [&](const double2 *Yc, const double2 *Yr, const unsigned *ens, size_t n, size_t row0, size_t max_rows) {
		                   return wx_pass(pl, call, who, P, h_bands, R, Yc, Yr, ens, n, row0, z, max_rows, d_sums, d_fit);
	                   });
}

extern "C" int tspws_hip_wxs_rows_stats(const tspws_hip_plan *pl, tspws_hip_wxs_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "wxs_rows_stats: NULL");
	*stats = pl->wxs_stats;
	return 0;
}
