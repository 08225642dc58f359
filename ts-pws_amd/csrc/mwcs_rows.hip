// mwcs_rows.hip -- dv/v by the moving-window cross-spectrum (tspws_hip_mwcs_rows; Clarke et al. 2011): every stack row of B ensembles against
// its ensemble's reference row, in windows of L samples every hop samples inside W lag ranges.  Per window the band-limited DFT of the
// demeaned, tapered row and reference, the smoothed cross-spectrum, its coherence and phase, and the weighted regression of the phase on the
// angular frequency (the delay); per (row, range) the weighted regression of the delays on the lag (dv/v).  Rows are what the batched calls
// write ([B][M][ld] floats, [B][M] host counts).
//
// Stage 1 is a dense FP64 contraction, (items x L samples) . (L x 2 Qx table columns), on the matrix pipe.
//   host         mwcs_plan.h: parameters, bins, windows, the basis table, rounds of whole ensembles inside TSPWS_PART_MB, per round ONE table
//                block and one upload
//   k_mw_dft     one WAVE per (tile of up to 32 items, group of up to 4 tiles of 16 columns, the tiles dealt evenly to the groups): an item is (row or reference, window), its L
//                consecutive floats at an unaligned base are the A operand (16 items x 4 samples) of v_mfma_f64_16x16x4_f64, the table (column
//                major, rows padded with zeros to a multiple of 16) the B operand; 2 x 4 independent accumulator tiles.  As in k_sr_dots a lane
//                loads four CONSECUTIVE samples of its item and of its column per block of 16 and feeds them to four steps.  L <= 1024: one wave
//                covers all of l.  The item's sum comes from the same registers; F = acc - (sum / L) T.  Items past the last re-read the last
//                item and store nothing; samples past L are never read (index 0 of the window is, and counts as zero).
//   k_mw_window  one WAVE per item, a lane per bin of [qa, qb): cross-spectrum and powers, the smoothing by shuffles in ascending d, coherence
//                and phase, then the sums over the band in ascending q (every lane runs the same serial sum on values read with v_readlane); lane 0 writes delta, err, mcoh.
//                The waves of the reference items only copy their spectrum out when asked.
//   k_mw_fit     one WAVE per (row, range): the windows' results in chunks of 64, lane 0 adds them in ascending j and forms the two fits; the
//                rows left out get NaN (all lanes fill the optional outputs)
// Nothing is atomic, every output has one writer, every sum has one order that depends on the row, its reference, the window and the
// parameters alone: a repeated call is bit-identical, and B, M, the other ranges, the rounds and a tile's padding change no bit.
#include "tspws_internal.h"
#include "batch_host.h"
#include "mwcs_plan.h"

static_assert(sizeof(MwPar) == sizeof(tspws_mwcs_par) && sizeof(MwWin) == 8 && sizeof(MwSrc) == 8, "the tables' layout");

typedef double mw_v4d __attribute__((ext_vector_type(4)));

// the value lane q holds, for a wave-uniform q: two v_readlane_b32, no LDS traffic (what __shfl would cost)
__device__ __forceinline__ double mw_lane(double x, unsigned q)
{
	const long long b = __double_as_longlong(x);
	const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, (int)q), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), (int)q);
	return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// F[(slot J + j) Qp + c] for the items of tile t and the columns of group cg
__global__ void __launch_bounds__(256) k_mw_dft(const float *__restrict__ rows, size_t ld, const float *__restrict__ ref, size_t ldr, const MwSrc *__restrict__ srcs,
                                                const MwWin *__restrict__ wins, unsigned J, unsigned L, unsigned Lp, const double *__restrict__ Bt,
                                                const double *__restrict__ T, unsigned Qp, unsigned ncg, unsigned long long nitems, unsigned long long nwaves,
                                                double *__restrict__ F)
{
#pragma clang fp contract(off)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long work = (unsigned long long)blockIdx.x * 4 + wave;
	if (work >= nwaves) return; // (the whole wave)
	const unsigned cg = (unsigned)(work % ncg);
	const unsigned long long item0 = work / ncg * MW_ROWS;
	const unsigned li = lane & 15, lk = lane >> 4;
	// the tiles of 16 columns are dealt evenly to the groups: group cg takes the tiles [t0, t0 + ntl), 1 <= ntl <= MW_NT (ncg = ceil(tiles / MW_NT))
	const unsigned nct = Qp / MW_CT, per = (nct + ncg - 1) / ncg, t0 = cg * per, ntl = min(per, nct - t0);

	const float *ap[2];
#pragma unroll
	for (int rt = 0; rt < 2; rt++) {
		const unsigned long long id = min(item0 + (unsigned)rt * 16 + li, nitems - 1); // (items past the last: the last again, not stored)
		const MwSrc sc = srcs[id / J];
		const MwWin wn = wins[id % J];
		ap[rt] = (sc.bl == MW_REF ? ref + (size_t)sc.row * ldr : rows + (size_t)sc.row * ld) + wn.n0;
	}
	const double *bp[MW_NT];
	double tc[MW_NT];
#pragma unroll
	for (int nt = 0; nt < MW_NT; nt++) {
		const unsigned col = (t0 + ((unsigned)nt < ntl ? (unsigned)nt : ntl - 1)) * MW_CT + li; // (tiles past the group: its last tile again, neither multiplied nor stored)
		bp[nt] = Bt + (size_t)col * Lp;
		tc[nt] = T[col];
	}

	mw_v4d acc[2][MW_NT];
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int nt = 0; nt < MW_NT; nt++) acc[rt][nt] = (mw_v4d){0, 0, 0, 0};
	double sx[2] = {0.0, 0.0};

	float a[2][4];
	mw_v4d b[MW_NT];
	// the four samples of this lane in block blk: l = 16 blk + 4 lk .. + 3 (what lies past L counts as zero; the table's rows there are zero too)
	auto request = [&](const unsigned blk) {
		const unsigned c = 16 * blk + 4 * lk;
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int q = 0; q < 4; q++) a[rt][q] = ap[rt][c + (unsigned)q < L ? c + (unsigned)q : 0u];
#pragma unroll
		for (int nt = 0; nt < MW_NT; nt++) b[nt] = *(const mw_v4d *)(bp[nt] + c); // (c + 3 < Lp: Lp is a multiple of 16)
	};
	const unsigned nblk = Lp / 16;
	request(0);
	for (unsigned blk = 0; blk < nblk; blk++) {
		const unsigned c = 16 * blk + 4 * lk;
		double ad[2][4];
		mw_v4d bd[MW_NT];
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int q = 0; q < 4; q++) ad[rt][q] = c + (unsigned)q < L ? (double)a[rt][q] : 0.0;
#pragma unroll
		for (int nt = 0; nt < MW_NT; nt++) bd[nt] = b[nt];
		if (blk + 1 < nblk) request(blk + 1); // (wave-uniform)
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int q = 0; q < 4; q++) sx[rt] = fma(ad[rt][q], 1.0, sx[rt]);
#pragma unroll
		for (int nt = 0; nt < MW_NT; nt++)
			if ((unsigned)nt < ntl) { // (wave-uniform)
#pragma unroll
				for (int q = 0; q < 4; q++)
#pragma unroll
					for (int rt = 0; rt < 2; rt++) acc[rt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[rt][q], bd[nt][q], acc[rt][nt], 0, 0, 0);
			}
	}

	// the items' sums: lane (li, lk) holds the samples 4 lk .. of every block of item li; after the two steps every lane of item li holds its sum
#pragma unroll
	for (int rt = 0; rt < 2; rt++) {
		sx[rt] += __shfl_xor(sx[rt], 16, 64);
		sx[rt] += __shfl_xor(sx[rt], 32, 64);
	}
	// result register q of a tile: row 4 q + lk, column li (tools/probes/mfma_f64_layout.hip)
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const unsigned r = 4 * (unsigned)q + lk;
			const double mu = __shfl(sx[rt], (int)r, 64) / (double)L; // (lane r: li == r)
			const unsigned long long id = item0 + (unsigned)rt * 16 + r;
			if (id < nitems) {
				double *__restrict__ d = F + id * Qp + (size_t)t0 * MW_CT + li;
#pragma unroll
				for (int nt = 0; nt < MW_NT; nt++)
					if ((unsigned)nt < ntl) d[nt * MW_CT] = acc[rt][nt][q] - mu * tc[nt];
			}
		}
}

// win[(slot J + j) 3 ..] = delta, err, mcoh of every (row, window) of the round; d_win / d_spec (when given) from row b0 M on, d_spec_ref likewise
__global__ void __launch_bounds__(256) k_mw_window(const double *__restrict__ F, unsigned Qp, unsigned Qx, unsigned qlo, unsigned nq, int h,
                                                   const double *__restrict__ ksm, const double *__restrict__ vtab, const MwSrc *__restrict__ srcs, unsigned nrows,
                                                   unsigned J, unsigned long long nwork, double *__restrict__ win, double *__restrict__ d_win,
                                                   double2 *__restrict__ d_spec, double2 *__restrict__ d_spec_ref)
{
#pragma clang fp contract(off) // every operation of the definition is rounded on its own
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long work = (unsigned long long)blockIdx.x * 4 + wave; // = slot J + j
	if (work >= nwork) return; // (the whole wave)
	const unsigned slot = (unsigned)(work / J), j = (unsigned)(work % J);
	const MwSrc sc = srcs[slot];
	const bool in = lane < Qx;
	const double *__restrict__ fc = F + work * Qp;
	const double cr = in ? fc[lane] : 0.0, ci = in ? fc[Qx + lane] : 0.0;
	if (sc.bl == MW_REF) { // a reference's item
		if (d_spec_ref && in) d_spec_ref[((size_t)sc.row * J + j) * Qx + lane] = make_double2(cr, ci);
		return;
	}
	const double *__restrict__ fr = F + ((size_t)(nrows + sc.bl) * J + j) * Qp;
	const double rr = in ? fr[lane] : 0.0, ri = in ? fr[Qx + lane] : 0.0;
	const size_t o = (size_t)sc.row * J + j;
	if (d_spec && in) d_spec[o * Qx + lane] = make_double2(cr, ci);
	const double xr = cr * rr + ci * ri, xi = ci * rr - cr * ri, pc = cr * cr + ci * ci, pr = rr * rr + ri * ri;
	double sxr = 0.0, sxi = 0.0, spc = 0.0, spr = 0.0, ks = 0.0;
	for (int d = -h; d <= h; d++) { // (wave-uniform)
		const int from = (int)lane + d;
		const bool ok = from >= 0 && from < (int)Qx;
		const int fl = ok ? from : (int)lane;
		const double vxr = __shfl(xr, fl, 64), vxi = __shfl(xi, fl, 64), vpc = __shfl(pc, fl, 64), vpr = __shfl(pr, fl, 64);
		if (ok) {
			const double kd = ksm[d + h];
			sxr += kd * vxr; sxi += kd * vxi; spc += kd * vpc; spr += kd * vpr; ks += kd;
		}
	}
	sxr = sxr / ks; sxi = sxi / ks; spc = spc / ks; spr = spr / ks; // (k[0] = 1: ks >= 1)
	const bool band = lane >= qlo && lane < qlo + nq;
	const double am = hypot(sxr, sxi), pp = spc * spr;
	const double coh = am / sqrt(pp), phi = atan2(sxi, sxr), v = in ? vtab[lane] : 0.0;
	const double cc = coh < 0.99 ? coh : 0.99, c2 = cc * cc;
	const double wq = sqrt(c2 / (1.0 - c2) * sqrt(am)), wv = wq * v;
	const double t1 = wv * v, t2 = wv * phi, t3 = wv * wv;
	const bool dead = __ballot(band && pp == 0.0) != 0ull;
	double svv = 0.0, svp = 0.0, sw2 = 0.0, sc_ = 0.0;
	for (unsigned q = qlo; q < qlo + nq; q++) {
		svv += mw_lane(t1, q); svp += mw_lane(t2, q); sw2 += mw_lane(t3, q); sc_ += mw_lane(coh, q);
	}
	const double delta = svp / svv;
	const double res = phi - delta * v, r2 = res * res;
	double sr = 0.0;
	for (unsigned q = qlo; q < qlo + nq; q++) sr += mw_lane(r2, q);
	if (lane != 0) return;
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	const double s2 = sr / (double)(nq - 1);
	const double o0 = dead ? nan : delta, o1 = dead ? nan : sqrt(sw2 * s2) / svv, o2 = dead ? nan : sc_ / (double)nq;
	double *__restrict__ w = win + work * 3;
	w[0] = o0; w[1] = o1; w[2] = o2;
	if (d_win) { d_win[o * 3] = o0; d_win[o * 3 + 1] = o1; d_win[o * 3 + 2] = o2; }
}

// fit[((b0 M + rw) W + w) 6 ..] of every (row, range) of the round; NaN in d_win / d_spec for the rows left out
__global__ void __launch_bounds__(256) k_mw_fit(const double *__restrict__ win, const MwWin *__restrict__ wins, const unsigned *__restrict__ slot_of, unsigned J,
                                                unsigned W, unsigned j0_0, unsigned j0_1, unsigned j0_2, unsigned j0_3, unsigned j0_4, unsigned L, unsigned Qx, double z,
                                                double min_coh, double max_err, double max_delta, double err_floor, size_t row0, unsigned long long nwork,
                                                double *__restrict__ d_win, double *__restrict__ d_spec, double *__restrict__ fit)
{
#pragma clang fp contract(off)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long work = (unsigned long long)blockIdx.x * 4 + wave;
	if (work >= nwork) return; // (the whole wave)
	const unsigned w = (unsigned)(work % W);
	const size_t rw = (size_t)(work / W), row = row0 + rw;
	const unsigned slot = slot_of[rw];
	const unsigned ja = w == 0 ? j0_0 : w == 1 ? j0_1 : w == 2 ? j0_2 : j0_3;
	const unsigned jb = w == 0 ? j0_1 : w == 1 ? j0_2 : w == 2 ? j0_3 : j0_4;
	const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
	double *__restrict__ fo = fit + (row * W + w) * 6;
	if (slot == NOSLOT) { // the row does not take part
		if (d_win)
			for (size_t i = (size_t)ja * 3 + lane; i < (size_t)jb * 3; i += 64) d_win[row * J * 3 + i] = nan;
		if (d_spec)
			for (size_t i = (size_t)ja * Qx * 2 + lane; i < (size_t)jb * Qx * 2; i += 64) d_spec[row * J * Qx * 2 + i] = nan;
		if (lane == 0) { fo[0] = nan; fo[1] = nan; fo[2] = nan; fo[3] = nan; fo[4] = nan; fo[5] = -1.0; }
		return;
	}
	double S = 0.0, St = 0.0, Stt = 0.0, Sd = 0.0, Std = 0.0, n = 0.0;
	for (unsigned jc = ja; jc < jb; jc += 64) { // (wave-uniform) a chunk of 64 windows: a lane loads one, lane 0 adds them in ascending j
		const unsigned jm = jc + lane < jb ? jc + lane : jb - 1;
		const double *__restrict__ p = win + ((size_t)slot * J + jm) * 3;
		const double delta = p[0], err = p[1], mcoh = p[2];
		const double t = ((double)wins[jm].n0 + 0.5 * (double)(L - 1)) - z;
		const bool take = fabs(delta) < inf && fabs(err) < inf && err <= max_err && mcoh >= min_coh && fabs(delta) <= max_delta;
		const double e = err > err_floor ? err : err_floor, pw = 1.0 / (e * e), pt = pw * t;
		const double a0 = pw, a1 = pt, a2 = pt * t, a3 = pw * delta, a4 = pt * delta;
		const unsigned cnt = min(64u, jb - jc);
		for (unsigned i = 0; i < cnt; i++) {
			const double b0 = mw_lane(a0, i), b1 = mw_lane(a1, i), b2 = mw_lane(a2, i), b3 = mw_lane(a3, i), b4 = mw_lane(a4, i);
			if (__builtin_amdgcn_readlane((int)take, (int)i)) { S += b0; St += b1; Stt += b2; Sd += b3; Std += b4; n += 1.0; } // (wave-uniform)
		}
	}
	if (lane != 0) return;
	const double den = S * Stt - St * St;
	double eh = nan, ic = nan, ee = nan, e0 = nan, r0 = nan;
	if (n >= 2.0 && den > 0.0) {
		eh = (S * Std - St * Sd) / den;
		ic = (Stt * Sd - St * Std) / den;
		ee = sqrt(S / den);
	}
	if (n >= 1.0 && Stt > 0.0) {
		e0 = Std / Stt;
		r0 = sqrt(1.0 / Stt);
	}
	fo[0] = eh; fo[1] = ic; fo[2] = ee; fo[3] = e0; fo[4] = r0; fo[5] = n;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
extern "C" int tspws_mwcs_bins(unsigned P, double dt, double f_lo, double f_hi, unsigned *q0, unsigned *q1)
{
	if (!q0 || !q1) return 1;
	if (P < MW_LMIN || P > MW_PMAX || (P & (P - 1)) || !(dt > 0.0) || !std::isfinite(dt) || !(f_lo >= 0.0) || !(f_hi > f_lo) || !std::isfinite(f_hi)) return 2;
	// bin q sits at q / (P dt): the bins with f_lo <= q / (P dt) < f_hi, without bin 0 and up to P / 2 - 1
	const double s = (double)P * dt, a = ceil(f_lo * s), b = ceil(f_hi * s);
	const unsigned lo = a < 1.0 ? 1u : a > (double)(P / 2) ? P / 2 : (unsigned)a, hi = b > (double)(P / 2) ? P / 2 : (unsigned)b;
	if (hi < 2 || lo > hi - 2) return 3; // fewer than two bins
	*q0 = lo; *q1 = hi;
	return 0;
}

extern "C" size_t tspws_mwcs_basis_size(const tspws_mwcs_par *par)
{
	if (!par || mw_par_error(*(const MwPar *)par)) return 0;
	return mw_basis_layout(*(const MwPar *)par).doubles;
}

extern "C" int tspws_mwcs_basis(const tspws_mwcs_par *par, double *tab)
{
	if (!par || !tab) return 1;
	if (mw_par_error(*(const MwPar *)par)) return 2;
	mw_basis(*(const MwPar *)par, tab);
	return 0;
}

extern "C" int tspws_hip_mwcs_rows(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                                   size_t ldr, double z, const tspws_mwcs_par *par, const size_t *h_win, unsigned W, double *d_win, double *d_fit, double *d_spec,
                                   double *d_spec_ref, void *s)
{
	// first what needs no plan
	if (!d_rows || !d_ref || !par || !h_win || !d_fit) return fail(TSPWS_E_ARG, "mwcs_rows: NULL");
	const MwPar P = *(const MwPar *)par;
	if (const char *e = mw_par_error(P)) return refuse("mwcs_rows", e);
	if (const char *e = range_error(h_win, W, LAG_RANGES)) return refuse("mwcs_rows", e);
	if (!std::isfinite(z)) return fail(TSPWS_E_ARG, "mwcs_rows: a NaN or infinite zero-lag position");
	const unsigned long long Jn = mw_count_windows(h_win, W, P.L, P.hop);
	if (!Jn) return fail(TSPWS_E_ARG, "mwcs_rows: no lag range holds a window");
	if (Jn > MW_JMAX) return fail(TSPWS_E_ARG, "mwcs_rows: more than 4096 windows");
	if (!pl) return fail(TSPWS_E_ARG, "mwcs_rows: NULL");
	const size_t N = pl->N;
	if (ld < N) return fail(TSPWS_E_ARG, "mwcs_rows: row stride below the trace length");
	if (ldr < N) return fail(TSPWS_E_ARG, "mwcs_rows: reference row stride below the trace length");
	if (const char *e = range_past_error(h_win, W, N, LAG_RANGES)) return refuse("mwcs_rows", e);
	if (!B || !M) return 0;
	if ((unsigned long long)B * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "mwcs_rows: more than 2^32 - 16 rows");

	const unsigned J = (unsigned)Jn;
	const MwBins bins = mw_bins(P);
	const MwWins wl = mw_windows(h_win, W, P.L, P.hop);
	std::vector<double> basis(mw_basis_layout(P).doubles);
	mw_basis(P, basis.data());
	const std::vector<size_t> nrows0 = participating_rows0(h_mtr, B, M);
	const std::vector<Round> rounds = mw_rounds(B, nrows0.data(), M, J, P, tspws_part_budget_bytes());
	const unsigned ncg = (bins.Qp / MW_CT + MW_NT - 1) / MW_NT;
	size_t max_tab = 0, max_spec = 0, max_win = 0;
	for (const Round &r : rounds) {
		const size_t nb = r.j1 - r.j0, nrows = nrows0[r.j1] - nrows0[r.j0];
		// one workgroup per 4 waves: the grids of the three launches
		const unsigned long long waves = std::max({((unsigned long long)(nrows + nb) * J + MW_ROWS - 1) / MW_ROWS * ncg, (unsigned long long)(nrows + nb) * J,
		                                           (unsigned long long)nb * M * W});
		if ((waves + 3) / 4 > 0x7fffffffull) return fail(TSPWS_E_ARG, "mwcs_rows: more than 2^33 waves in a round");
		max_tab = std::max(max_tab, mw_tab(P, J, nrows + nb, nb * M).bytes);
		max_spec = std::max(max_spec, mw_spec_bytes(nb, nrows, J, bins));
		max_win = std::max(max_win, mw_win_bytes(nrows, J));
	}

	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_mwcs_stats &stats = pl->mwcs_stats;
	stats = tspws_hip_mwcs_stats();
	stats.rows = (unsigned)nrows0[B];
	stats.left_out = (unsigned)((size_t)B * M - nrows0[B]);
	stats.windows = J;
	stats.bins = bins.Qx;
	BatchCall call(st);
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_MWF, std::max<size_t>(max_spec, 16), &v))) return rc; // (the largest round's: the slots do not grow between rounds)
	double *F = (double *)v;
	if ((rc = scratch(pl, SCR_MWW, std::max<size_t>(max_win, 16), &v))) return rc;
	double *win = (double *)v;
	for (const Round &r : rounds) {
		const size_t nb = r.j1 - r.j0, nrows = nrows0[r.j1] - nrows0[r.j0], row0 = r.j0 * (size_t)M;
		stats.rounds++;
		const MwTab o = mw_tab(P, J, nrows + nb, nb * M);
		char *blob = call.block(o.bytes), *tab;
		mw_fill_round(blob, o, r, M, h_mtr, P, basis.data(), wl);
		if ((rc = call.upload(pl, SCR_MWTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const MwSrc *d_srcs = (const MwSrc *)(tab + o.srcs);
		const MwWin *d_wins = (const MwWin *)(tab + o.wins);
		const unsigned long long nitems = (unsigned long long)(nrows + nb) * J, n1 = (nitems + MW_ROWS - 1) / MW_ROWS * ncg;
		hipLaunchKernelGGL(k_mw_dft, dim3((unsigned)((n1 + 3) / 4)), dim3(256), 0, st, d_rows, ld, d_ref, ldr, d_srcs, d_wins, J, P.L, bins.Lp,
		                   (const double *)(tab + o.bt), (const double *)(tab + o.T), bins.Qp, ncg, nitems, n1, F);
		hipLaunchKernelGGL(k_mw_window, dim3((unsigned)((nitems + 3) / 4)), dim3(256), 0, st, (const double *)F, bins.Qp, bins.Qx, P.q0 - bins.qa, P.q1 - P.q0, (int)P.h,
		                   (const double *)(tab + o.k), (const double *)(tab + o.v), d_srcs, (unsigned)nrows, J, nitems, win, d_win, (double2 *)d_spec,
		                   (double2 *)d_spec_ref);
		const unsigned long long n3 = (unsigned long long)nb * M * W;
		hipLaunchKernelGGL(k_mw_fit, dim3((unsigned)((n3 + 3) / 4)), dim3(256), 0, st, (const double *)win, d_wins, (const unsigned *)(tab + o.slot_of), J, W, wl.j0[0],
		                   wl.j0[1], wl.j0[2], wl.j0[3], wl.j0[4], P.L, bins.Qx, z, P.min_coh, P.max_err, P.max_delta, P.err_floor, row0, n3, d_win, d_spec, d_fit);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_mwcs_rows_stats(const tspws_hip_plan *pl, tspws_hip_mwcs_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "mwcs_rows_stats: NULL");
	*stats = pl->mwcs_stats;
	return 0;
}
