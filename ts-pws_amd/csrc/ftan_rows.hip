// ftan_rows.hip -- group arrivals per scale from stack rows (tspws_hip_ftan_coef, tspws_hip_ftan_rows): frequency-time analysis on the frame's
// own coefficients.  Per (row, window, scale) the local maxima of the squared envelope a2[k] = |Y_s[k]|^2 among the window's members, the
// first P of them by decreasing a2, each with its three-point vertex, the coefficient at the peak and its index; per (row, scale) the sum
// and the number of the finite a2 inside a noise range.  Rows are what the batched calls write ([B][M][ld] floats, [B][M] host counts);
// windows and noise ranges are per ensemble.  tspws_hip_ftan_rows transforms the rows in rounds with tspws_hip_forward_f32.
//
//   host         ftan_plan.h: the classes of ensembles with equal windows, per class the items (segments of FT_SEG members of one scale and
//                window, or of one scale and the noise range), the tasks (runs of short items), the rounds, ONE table block and one upload
//                per pass
//   k_ft_reduce  one WAVE per (participating row, task): item after item, the lanes read consecutive complex coefficients (16 B per lane,
//                1 KB per wave and load; the next pass's loads are in flight while a pass computes) and form a2; the neighbours' a2 come
//                from the adjacent lanes, those of the pass's first and last lane from one halo coefficient each.  A lane keeps the peak of
//                each of the item's 4 passes; the wave selects the item's first P by P rounds of a fixed 64-lane max-reduction on the key
//                (bits of a2, smaller k wins: a2 is finite and positive, so its bit pattern orders as an integer) and leaves P x (a2, k) per
//                item.  A noise item adds a2 per lane in increasing k, reduces through valu_reduce16 and leaves (Q, n).
//   k_ft_final   one thread per (row, window, scale): merges the segments' lists in segment order into the first P, reads c[k-1], c[k],
//                c[k+1] of the round's set, recomputes the three a2 (the same bits) and writes the five values; one thread per (row,
//                scale) adds the noise partials in increasing segment order; NaN and -1 for the rows left out
// Nothing is atomic, every output has one writer, and what (row, window, scale) gets depends on that scale's coefficients, the window, z and
// the wrap rule alone: a repeated call is bit-identical, and B, M, the other windows, scales and ensembles, P, the rounds and the padding
// change no bit.
#include "tspws_internal.h"
#include "coef_rows.h"
#include "lane_reduce.h"
#include "ftan_plan.h"

static_assert(sizeof(FtItem) == 24 && sizeof(FtClass) == 16 && sizeof(FtScale) == 16 && FT_SEG == 4 * 64 && FT_PMAX == 4, "the tables' layout");

__device__ __forceinline__ bool ft_finite(double x) { return (__double_as_longlong(x) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }

// part[(slot max_items + item of the class) P + r] = (bits of a2, k) of the item's r-th peak ((0, -1): none), or (Q, n) in r = 0 of a noise item
__global__ void __launch_bounds__(256) k_ft_reduce(const double2 *__restrict__ Y, size_t ncoef, const FtItem *__restrict__ items, const FtTask *__restrict__ tasks,
                                                   const FtClass *__restrict__ classes, const FtRow *__restrict__ list, unsigned max_items, unsigned max_tasks,
                                                   unsigned P, unsigned long long nwork, ulonglong2 *__restrict__ part)
{
#pragma clang fp contract(off) // every operation of the definition is rounded on its own
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long work = (unsigned long long)blockIdx.x * 4 + wave;
	if (work >= nwork) return; // (the whole wave)
	const unsigned t = (unsigned)(work % max_tasks);
	const size_t slot = (size_t)(work / max_tasks);
	const FtRow rw = list[slot];
	const FtClass cl = classes[rw.cls];
	if (t >= cl.ntasks) return; // (a class with fewer tasks than the largest)
	const double2 *__restrict__ y = Y + (size_t)rw.row * ncoef;
	const FtTask tk = tasks[cl.task0 + t];
	const bool edge = lane == 0 || lane == 63;
	for (unsigned i = tk.first; i < tk.first + tk.n; i++) {
		const FtItem it = items[i];
		const double2 *__restrict__ ys = y + it.base;
		ulonglong2 *__restrict__ out = part + ((size_t)slot * max_items + (i - cl.item0)) * P;
		const unsigned npass = (it.count + 63) / 64, last = it.Ns - 1; // (wave-uniform; an item holds at least one member)
		if (it.noise) {
			double v[16];
#pragma unroll
			for (int e = 0; e < 16; e++) v[e] = 0.0;
			double2 c = ys[it.k0 + (lane < it.count ? lane : 0u)];
#pragma unroll 1
			for (unsigned p = 0; p < npass; p++) {
				const unsigned j = lane + 64 * p, jn = j + 64;
				const double2 cn = ys[it.k0 + (jn < it.count ? jn : 0u)];
				const double a0 = c.x * c.x + c.y * c.y;
				if (j < it.count && ft_finite(a0)) { v[0] += a0; v[1] += 1.0; }
				c = cn;
			}
			const double sum = valu_reduce16(v, lane); // element 0 in lanes 0 .. 3, element 1 in lanes 4 .. 7
			if (lane == 0) ((double *)out)[0] = sum;
			if (lane == 4) ((double *)out)[1] = sum;
			continue;
		}
		// pass p: index k0 + lane + 64 p of the scale (an index past the scale's end reads its last coefficient and is no member); the first
		// lane also reads index k - 1, the last one k + 1; the next pass's loads are in flight while this one computes
		unsigned long long key[4];
		const unsigned kl = it.k0 + lane;
		double2 c = ys[kl < last ? kl : last];
		double2 h = c;
		if (edge) h = ys[lane == 0 ? (kl ? kl - 1 : 0u) : (kl + 1 < last ? kl + 1 : last)];
#pragma unroll
		for (unsigned p = 0; p < 4; p++) {
			key[p] = 0;
			if (p < npass) { // (wave-uniform)
				const unsigned j = lane + 64 * p, k = it.k0 + j;
				double2 cn = c, hn = h;
				if (p + 1 < npass) {
					const unsigned kn = k + 64;
					cn = ys[kn < last ? kn : last];
					if (edge) hn = ys[lane == 0 ? kn - 1 : (kn + 1 < last ? kn + 1 : last)];
				}
				const double a0 = c.x * c.x + c.y * c.y, ah = h.x * h.x + h.y * h.y;
				double am = __shfl_up(a0, 1), ap = __shfl_down(a0, 1);
				if (lane == 0) am = ah;
				if (lane == 63) ap = ah;
				const bool peak = j < it.count && k >= 1 && k < last && ft_finite(am) && ft_finite(a0) && ft_finite(ap) && a0 > am && a0 >= ap;
				key[p] = peak ? (unsigned long long)__double_as_longlong(a0) : 0ull;
				c = cn; h = hn;
			}
		}
		// the item's first P peaks: P rounds of one fixed 64-lane max-reduction on (key, smaller k wins); every lane ends with the winner
		for (unsigned r = 0; r < P; r++) {
			unsigned long long bk = key[0];
			unsigned bp = 0;
#pragma unroll
			for (unsigned p = 1; p < 4; p++)
				if (key[p] > bk) { bk = key[p]; bp = p; }
			unsigned bi = kl + 64 * bp;
#pragma unroll
			for (int m = 32; m >= 1; m >>= 1) {
				const unsigned long long ok = __shfl_xor(bk, m);
				const unsigned oi = __shfl_xor(bi, m);
				if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
			}
			const bool some = __builtin_amdgcn_readfirstlane((int)(bk != 0)) != 0;
			if (lane == 0) out[r] = make_ulonglong2(bk, some ? (unsigned long long)bi : ~0ull);
			if (!some) { // no peak is left: the other slots are empty too
				if (lane == 0)
					for (unsigned q = r + 1; q < P; q++) out[q] = make_ulonglong2(0ull, ~0ull);
				break;
			}
#pragma unroll
			for (unsigned p = 0; p < 4; p++)
				if (bi == kl + 64 * p) key[p] = 0;
		}
	}
}

// peaks[((row0 + row) W + w) Sx + sx][P][5] of every (row, window, scale) of the pass, then noise[(row0 + row) Sx + sx][2] of every (row, scale)
__global__ void __launch_bounds__(256) k_ft_final(const double2 *__restrict__ Y, size_t ncoef, const ulonglong2 *__restrict__ part, const FtClass *__restrict__ classes,
                                                  const FtSpan *__restrict__ pspans, const FtSpan *__restrict__ nspans, const FtScale *__restrict__ scales,
                                                  const FtRow *__restrict__ list, const unsigned *__restrict__ slot_of, unsigned W, unsigned Sx, unsigned P,
                                                  unsigned max_items, double z, size_t row0, unsigned long long npk, unsigned long long nout,
                                                  double *__restrict__ peaks, double *__restrict__ noise)
{
#pragma clang fp contract(off)
	const unsigned long long o = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (o >= nout) return;
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	if (o >= npk) { // the noise level of (row, scale)
		const unsigned long long on = o - npk;
		const unsigned sx = (unsigned)(on % Sx);
		const size_t row = (size_t)(on / Sx);
		double *__restrict__ no = noise + ((size_t)row0 * Sx + on) * 2;
		const unsigned slot = slot_of[row];
		if (slot == NOSLOT) { no[0] = nan; no[1] = -1.0; return; }
		const FtRow rw = list[slot];
		const FtClass cl = classes[rw.cls];
		const FtSpan sp = nspans[(size_t)rw.cls * Sx + sx];
		const ulonglong2 *__restrict__ pp = part + ((size_t)slot * max_items + (sp.first - cl.item0)) * P;
		double Q = 0.0, n = 0.0;
		for (unsigned i = 0; i < sp.n; i++) {
			const ulonglong2 e = pp[(size_t)i * P];
			Q += __longlong_as_double((long long)e.x);
			n += __longlong_as_double((long long)e.y);
		}
		no[0] = Q; no[1] = n;
		return;
	}
	const unsigned sx = (unsigned)(o % Sx), w = (unsigned)((o / Sx) % W);
	const size_t row = (size_t)(o / Sx / W);
	double *__restrict__ po = peaks + ((size_t)row0 * W * Sx + o) * P * 5;
	const unsigned slot = slot_of[row];
	unsigned long long bk[4] = {0, 0, 0, 0}, bi[4] = {0, 0, 0, 0}; // the first peaks so far, by (a2 decreasing, k increasing)
	const double2 *__restrict__ ys = Y;
	unsigned D = 0;
	if (slot != NOSLOT) {
		const FtRow rw = list[slot];
		const FtClass cl = classes[rw.cls];
		const FtSpan sp = pspans[((size_t)rw.cls * Sx + sx) * W + w];
		const FtScale sc = scales[sx];
		ys = Y + (size_t)rw.row * ncoef + sc.base;
		D = sc.D;
		const ulonglong2 *__restrict__ pp = part + ((size_t)slot * max_items + (sp.first - cl.item0)) * P;
		for (unsigned i = 0; i < sp.n; i++)
			for (unsigned r = 0; r < P; r++) {
				const ulonglong2 e = pp[(size_t)i * P + r];
				if (!e.x) break;
				unsigned long long nk = e.x, ni = e.y;
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (nk > bk[j] || (nk == bk[j] && nk && ni < bi[j])) {
						const unsigned long long tk = bk[j], ti = bi[j];
						bk[j] = nk; bi[j] = ni; nk = tk; ni = ti;
					}
			}
	}
#pragma unroll
	for (unsigned r = 0; r < 4; r++) {
		if (r >= P) break;
		double *__restrict__ q = po + r * 5;
		if (!bk[r]) { q[0] = nan; q[1] = nan; q[2] = nan; q[3] = nan; q[4] = -1.0; continue; }
		const size_t k = (size_t)bi[r];
		const double2 cm = ys[k - 1], c0 = ys[k], cp = ys[k + 1];
		const double am = cm.x * cm.x + cm.y * cm.y, a0 = c0.x * c0.x + c0.y * c0.y, ap = cp.x * cp.x + cp.y * cp.y;
		const double den = (am - 2.0 * a0) + ap;
		const double d = den != 0.0 ? 0.5 * (am - ap) / den : 0.0;
		q[0] = ((double)k + d) * (double)D - z;
		q[1] = sqrt(a0);
		q[2] = c0.x; q[3] = c0.y;
		q[4] = (double)k;
	}
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the checks both entry points share, in the contract's order: first what needs no plan (pl may be NULL there)
static int ft_check(const tspws_hip_plan *pl, const char *who, unsigned long long nrows, unsigned B, double z, unsigned s_begin, unsigned s_end, const size_t *win,
                    unsigned W, const size_t *noise, unsigned P, const double *d_noise)
{
	const std::string w(who);
	if (!pl) {
		if (const char *e = range_count_error(W, WINDOWS)) return refuse(who, e);
		if (!P || P > FT_PMAX) return fail(TSPWS_E_ARG, (w + ": 1 to 4 peaks").c_str());
		if (s_begin >= s_end) return fail(TSPWS_E_ARG, (w + ": an empty scale range (s_begin >= s_end)").c_str());
		if (d_noise && !noise) return fail(TSPWS_E_ARG, (w + ": a noise output without a noise range").c_str());
		if (!std::isfinite(z)) return fail(TSPWS_E_ARG, (w + ": a NaN or infinite zero-lag position").c_str());
		if (nrows > 0xfffffff0ull) return fail(TSPWS_E_ARG, (w + ": more than 2^32 - 16 rows").c_str()); // (from the counts alone: before a table is read)
		if (const char *e = range_empty_error(win, (size_t)B * W, WINDOWS)) return refuse(who, e);
		for (size_t b = 0; noise && b < B; b++)
			if (noise[2 * b] >= noise[2 * b + 1]) return fail(TSPWS_E_ARG, (w + ": an empty noise range (q0 >= q1)").c_str());
		return 0;
	}
	if (s_end > pl->S) return fail(TSPWS_E_ARG, (w + ": the scale range ends behind the last scale").c_str());
	if (const char *e = range_past_error(win, (size_t)B * W, pl->N, WINDOWS)) return refuse(who, e);
	for (size_t b = 0; noise && b < B; b++)
		if (noise[2 * b + 1] > pl->N) return fail(TSPWS_E_ARG, (w + ": a noise range past the trace length").c_str());
	return 0;
}

static FtPlan ft_plan_of(const tspws_hip_plan *pl, unsigned s_begin, unsigned s_end, const size_t *win, unsigned W, const size_t *noise, size_t B, int skip_wrapped)
{
	return ft_plan(wx_scales_of(pl).data(), pl->S, pl->N, s_begin, s_end, win, W, noise, B, skip_wrapped);
}

// one pass: the rows [0, nrows) of Y, ens[.] = the ensemble of every row (NOSLOT: the row does not take part); outputs from row `row0` on;
// the slots are reserved for a pass of max_rows rows
static int ft_pass(tspws_hip_plan *pl, BatchCall &call, const char *who, const FtPlan &F, unsigned P, const double2 *Y, const unsigned *ens, size_t nrows,
                   size_t row0, double z, size_t max_rows, double *d_peaks, double *d_noise)
{
	hipStream_t st = call.stream();
	const size_t nslots = count_slots(ens, nrows), max_tab = ft_tab(F, max_rows, max_rows).bytes, max_part = ft_part_bytes(F, P, max_rows);
	const FtTab o = ft_tab(F, nslots, nrows);
	const unsigned long long nwork = (unsigned long long)nslots * F.max_tasks, npk = (unsigned long long)nrows * F.W * F.Sx,
	                         nout = npk + (d_noise ? (unsigned long long)nrows * F.Sx : 0);
	if ((nwork + 3) / 4 > 0x7fffffffull || (nout + 255) / 256 > 0x7fffffffull) return fail(TSPWS_E_ARG, (std::string(who) + ": more than 2^33 waves in a round").c_str());
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_FTP, std::max<size_t>({ft_part_bytes(F, P, nslots), max_part, 16}), &v))) return rc;
	ulonglong2 *part = (ulonglong2 *)v;
	char *blob = call.block(o.bytes), *tab;
	ft_fill(blob, o, F, ens, nrows);
	if ((rc = call.upload(pl, SCR_FTTAB, blob, o.bytes, &tab, max_tab))) return rc;
	if (nwork)
		hipLaunchKernelGGL(k_ft_reduce, dim3((unsigned)((nwork + 3) / 4)), dim3(256), 0, st, Y, pl->ncoef, (const FtItem *)(tab + o.items),
		                   (const FtTask *)(tab + o.tasks), (const FtClass *)(tab + o.classes), (const FtRow *)(tab + o.list), F.max_items, F.max_tasks, P, nwork, part);
	hipLaunchKernelGGL(k_ft_final, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, Y, pl->ncoef, (const ulonglong2 *)part, (const FtClass *)(tab + o.classes),
	                   (const FtSpan *)(tab + o.pspans), (const FtSpan *)(tab + o.nspans), (const FtScale *)(tab + o.scales), (const FtRow *)(tab + o.list),
	                   (const unsigned *)(tab + o.slot_of), F.W, F.Sx, P, F.max_items, z, row0, npk, nout, d_peaks, d_noise);
	return 0;
}

static void ft_stats_begin(tspws_hip_plan *pl, const FtPlan &F)
{
	pl->ftan_stats = tspws_hip_ftan_stats();
	pl->ftan_stats.items = (unsigned)F.items.size();
	pl->ftan_stats.classes = (unsigned)F.classes.size();
}

extern "C" int tspws_hip_ftan_coef(tspws_hip_plan *pl, const double *d_Y, const unsigned *h_ens, size_t nrow, unsigned B, double z, unsigned s_begin, unsigned s_end,
                                   const size_t *h_win, unsigned W, const size_t *h_noise, unsigned P, int skip_wrapped, double *d_peaks, double *d_noise, void *s)
{
	const char *who = "ftan_coef";
	if (!d_Y || !h_win || !d_peaks) return fail(TSPWS_E_ARG, "ftan_coef: NULL");
	if (int rc = ft_check(nullptr, who, nrow, B, z, s_begin, s_end, h_win, W, h_noise, P, d_noise)) return rc;
	if (!pl) return fail(TSPWS_E_ARG, "ftan_coef: NULL");
	if (int rc = ft_check(pl, who, nrow, B, z, s_begin, s_end, h_win, W, h_noise, P, d_noise)) return rc;
	if (!nrow || !B) return 0;
	if (!h_ens && nrow != B) return fail(TSPWS_E_ARG, "ftan_coef: without h_ens the rows must number B");
	if (h_ens)
		for (size_t i = 0; i < nrow; i++)
			if (h_ens[i] >= B) return fail(TSPWS_E_ARG, "ftan_coef: an ensemble index >= B");

	const FtPlan F = ft_plan_of(pl, s_begin, s_end, h_win, W, d_noise ? h_noise : nullptr, B, skip_wrapped);
	const size_t chunk = ft_chunk_rows(nrow, F, P, tspws_part_budget_bytes());
	HIP_TRY(hipSetDevice(pl->device));
	BatchCall call(S_(s));
	ft_stats_begin(pl, F);
	return coef_chunks(call, row_counters(pl->ftan_stats), (const double2 *)d_Y, nullptr, pl->ncoef, h_ens, nrow, chunk,
	                   [&](const double2 *Y, const double2 *, const unsigned *ens, size_t n, size_t row0, size_t max_rows) {
		                   return ft_pass(pl, call, who, F, P, Y, ens, n, row0, z, max_rows, d_peaks, d_noise);
	                   });
}

extern "C" int tspws_hip_ftan_rows(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, double z, unsigned s_begin,
                                   unsigned s_end, const size_t *h_win, unsigned W, const size_t *h_noise, unsigned P, int skip_wrapped, double *d_peaks,
                                   double *d_noise, void *s)
{
	const char *who = "ftan_rows";
	if (!d_rows || !h_win || !d_peaks) return fail(TSPWS_E_ARG, "ftan_rows: NULL");
	if (int rc = ft_check(nullptr, who, (unsigned long long)B * M, B, z, s_begin, s_end, h_win, W, h_noise, P, d_noise)) return rc;
	if (!pl) return fail(TSPWS_E_ARG, "ftan_rows: NULL");
	if (ld < pl->N) return fail(TSPWS_E_ARG, "ftan_rows: row stride below the trace length");
	if (int rc = ft_check(pl, who, (unsigned long long)B * M, B, z, s_begin, s_end, h_win, W, h_noise, P, d_noise)) return rc;
	if (!B || !M) return 0;

	const FtPlan F = ft_plan_of(pl, s_begin, s_end, h_win, W, d_noise ? h_noise : nullptr, B, skip_wrapped);
	const std::vector<Round> rounds = ft_rounds(B, M, pl->ncoef, F, P, tspws_part_budget_bytes());
	HIP_TRY(hipSetDevice(pl->device));
	BatchCall call(S_(s));
	ft_stats_begin(pl, F);
	return coef_rounds(pl, call, row_counters(pl->ftan_stats), d_rows, ld, M, h_mtr, nullptr, 0, 0, rounds, SCR_FTY,
	                   [&](const double2 *Y, const double2 *, const unsigned *ens, size_t n, size_t row0, size_t max_rows) {
		                   return ft_pass(pl, call, who, F, P, Y, ens, n, row0, z, max_rows, d_peaks, d_noise);
	                   });
}

extern "C" int tspws_hip_ftan_rows_stats(const tspws_hip_plan *pl, tspws_hip_ftan_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "ftan_rows_stats: NULL");
	*stats = pl->ftan_stats;
	return 0;
}

// ---- host rules, no device -----------------------------------------------------------------------------------------------------------
extern "C" int tspws_ftan_windows(double dist, double vmin, double vmax, double dt, double z, size_t N, int sides, size_t *win)
{
	if (!win) return fail(TSPWS_E_ARG, "ftan_windows: NULL");
	if (sides != 1 && sides != 2) return fail(TSPWS_E_ARG, "ftan_windows: sides must be 1 or 2");
	if (!std::isfinite(dist) || !std::isfinite(vmin) || !std::isfinite(vmax) || !std::isfinite(dt) || !std::isfinite(z) || !(dist >= 0) || !(vmin > 0) ||
	    !(vmax >= vmin) || !(dt > 0))
		return fail(TSPWS_E_ARG, "ftan_windows: needs finite dist >= 0, 0 < vmin <= vmax, dt > 0 and z");
	const double near = dist / (vmax * dt), far = dist / (vmin * dt); // the lags of the fastest and the slowest arrival, in samples
	const double lo[2] = {std::ceil(z + near), std::ceil(z - far)}, hi[2] = {std::floor(z + far) + 1.0, std::floor(z - near) + 1.0};
	size_t out[4];
	for (int i = 0; i < sides; i++) {
		if (!std::isfinite(lo[i]) || !std::isfinite(hi[i])) return fail(TSPWS_E_ARG, "ftan_windows: a window edge is not finite");
		const double a = std::max(lo[i], 0.0), b = std::min(hi[i], (double)N);
		if (!(a < b)) return fail(TSPWS_E_ARG, "ftan_windows: an empty window");
		out[2 * i] = (size_t)a; out[2 * i + 1] = (size_t)b;
	}
	std::copy(out, out + 2 * sides, win);
	return 0;
}

extern "C" int tspws_ftan_periods(const double *scale, unsigned S, double w0, double dt, double *T)
{
	if ((!scale || !T) && S) return fail(TSPWS_E_ARG, "ftan_periods: NULL");
	if (!(dt > 0) || !std::isfinite(dt)) return fail(TSPWS_E_ARG, "ftan_periods: dt must be positive");
	if (!(w0 > 0) || !std::isfinite(w0)) return fail(TSPWS_E_ARG, "ftan_periods: w0 must be positive");
	for (unsigned s = 0; s < S; s++) T[s] = 2 * TSPWS_PI * dt * scale[s] / w0; // 1 / fc_s of tspws_bands_from_frequencies
	return 0;
}
