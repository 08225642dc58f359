// stretch_rows.hip -- dv/v by stretching (tspws_hip_stretch_rows): the correlation coefficient of every stack row of B ensembles with its
// ensemble's reference row evaluated at lag t (1 + eps), on a grid of E stretch factors and over W coda windows, and per (row, window) the
// maximum with a three-point fit.  Rows are what the batched calls write ([B][M][ld] floats, [B][M] host counts).
//
// The work is a dense FP64 contraction per ensemble, (M rows x n window samples) . (n x E stretched references), on the matrix pipe.
//   host         stretch_plan.h: the windows packed side by side in segments of SR_SEG samples, rounds of (whole ensembles x chunks of the
//                grid in multiples of 16) inside TSPWS_PART_MB, per round ONE table block and one upload
//   k_sr_stretch one WAVE per (ensemble, stretch, segment): S[ensemble][stretch][packed column] in FP64 by cubic convolution of the
//                reference (Keys, a = -1/2; samples outside [0, N) are zero), coalesced along the columns, zero in the pad columns and for the
//                pad stretches; the wave also leaves the segment's sum of S^2
//   k_sr_dots    one WAVE per (tile of up to 32 participating rows, group of up to 4 tiles of 16 stretches, segment): the rows' floats become
//                the A operand (16 rows x 4 samples) of v_mfma_f64_16x16x4_f64, S the B operand (4 samples x 16 stretches); 2 x 4 independent
//                accumulator tiles.  A lane loads four CONSECUTIVE samples of its row and of its stretch per block of 16 columns and feeds
//                them to four steps, so step t multiplies the samples 16 blk + 4 k + t (k = lane / 16) -- A and B agree, the sum is the same.
//                Rows past the tile's last re-read its last row and store nothing.  The rows' sum of squares comes from the same loads, in
//                the waves of the call's first group of stretches only.
//   k_sr_final   one WAVE per (row, window): a lane per stretch adds the segments' partial sums in segment order and forms
//                cc = dot / sqrt(sum c^2) / sqrt(sum S^2); the first index of the largest non-NaN cc by a fixed reduction; lane 0 the fit
// Nothing is atomic, every output has one writer, every sum has one order that depends on the row, its reference, z, eps_e and the window
// alone: a repeated call is bit-identical, and batching, the other rows, grid entries and windows, the rounds and the padding change no bit.
#include "tspws_internal.h"
#include "batch_host.h"
#include "stretch_plan.h"

enum { SR_NT = 4 }; // tiles of 16 stretches per wave

typedef double sr_v4d __attribute__((ext_vector_type(4)));

// S[(bl Ec + el) J + joff + c] for the stretches e0 + el of a chunk, el < Ec; ss[(bl epad + e) nseg + seg]
__global__ void __launch_bounds__(256) k_sr_stretch(const float *__restrict__ ref, size_t ldr, unsigned N, double z, const SrSeg *__restrict__ segs, unsigned nseg,
                                                    const double *__restrict__ eps, unsigned E, unsigned epad, unsigned e0, unsigned Ec, unsigned b0, size_t J,
                                                    unsigned long long nitems, double *__restrict__ S, double *__restrict__ ss)
{
#pragma clang fp contract(off) // every operation of the definition is rounded on its own
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long item = (unsigned long long)blockIdx.x * 4 + wave;
	if (item >= nitems) return; // (the whole wave)
	const unsigned seg = (unsigned)(item % nseg);
	const unsigned long long r = item / nseg;
	const unsigned el = (unsigned)(r % Ec), bl = (unsigned)(r / Ec), e = e0 + el;
	if (e >= epad) return; // (the last chunk of a grid that is no multiple of Ec: those columns of S are never read)
	const SrSeg sg = segs[seg];
	double *__restrict__ out = S + ((size_t)bl * Ec + el) * J + sg.joff;
	if (e >= E) { // a pad stretch: zero columns
		for (unsigned c = lane; c < sg.plen; c += 64) out[c] = 0.0;
		return;
	}
	const double ee = eps[e], hi = (double)N + 1.0;
	const float *__restrict__ rp = ref + (size_t)(b0 + bl) * ldr;
	double acc = 0.0;
	for (unsigned c = lane; c < sg.plen; c += 64) {
		double s = 0.0;
		if (c < sg.len) {
			const double n = (double)(sg.n0 + c);
			const double u = n + (n - z) * ee;
			if (u >= -2.0 && u < hi) { // (otherwise all four samples lie outside [0, N))
				const double fl = floor(u), f = u - fl;
				const long long i = (long long)fl;
				const double wm = ((-0.5 * f + 1.0) * f - 0.5) * f;
				const double w0 = (1.5 * f - 2.5) * f * f + 1.0;
				const double w1 = ((-1.5 * f + 2.0) * f + 0.5) * f;
				const double w2 = (0.5 * f - 0.5) * f * f;
				const double rm = (i - 1 >= 0 && i - 1 < (long long)N) ? (double)rp[i - 1] : 0.0;
				const double r0 = (i >= 0 && i < (long long)N) ? (double)rp[i] : 0.0;
				const double r1 = (i + 1 >= 0 && i + 1 < (long long)N) ? (double)rp[i + 1] : 0.0;
				const double r2 = (i + 2 >= 0 && i + 2 < (long long)N) ? (double)rp[i + 2] : 0.0;
				s = ((wm * rm + w0 * r0) + w1 * r1) + w2 * r2;
			}
		}
		out[c] = s;
		acc = fma(s, s, acc);
	}
	acc = wave_sum(acc);
	if (lane == 0) ss[((size_t)bl * epad + e) * nseg + seg] = acc;
}

// dots[((slot0 + r) nseg + seg) epad + e] for the rows r of tile t and the stretches of group eg of the chunk; xx[(slot0 + r) nseg + seg] when do_xx
__global__ void __launch_bounds__(256) k_sr_dots(const float *__restrict__ rows, size_t ld, size_t M, const SrSeg *__restrict__ segs, unsigned nseg,
                                                 const SrTile *__restrict__ tiles, unsigned ntiles, const unsigned *__restrict__ list, const double *__restrict__ S,
                                                 size_t J, unsigned e0, unsigned Ec, unsigned epad, unsigned neg, int do_xx, unsigned long long nitems,
                                                 double *__restrict__ dots, double *__restrict__ xxp)
{
#pragma clang fp contract(off)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long item = (unsigned long long)blockIdx.x * 4 + wave;
	if (item >= nitems) return; // (the whole wave)
	const unsigned t = (unsigned)(item % ntiles);
	const unsigned long long r1 = item / ntiles;
	const unsigned eg = (unsigned)(r1 % neg), seg = (unsigned)(r1 / neg);
	const unsigned li = lane & 15, lk = lane >> 4;
	const SrTile tl = tiles[t];
	const SrSeg sg = segs[seg];
	const unsigned count = (unsigned)__builtin_amdgcn_readfirstlane((int)tl.count);
	const unsigned ntl = min((unsigned)SR_NT, (min(Ec, epad - e0) / SR_ET) - eg * SR_NT); // tiles of stretches of this group (>= 1: neg counts them)
	const bool first = do_xx && eg == 0;

	const float *ap[2];
#pragma unroll
	for (int rt = 0; rt < 2; rt++) {
		const unsigned r = (unsigned)rt * 16 + li;
		ap[rt] = rows + ((size_t)tl.b * M + list[tl.slot0 + (r < count ? r : count - 1)]) * ld + sg.n0; // (rows past the tile: its last row again, not stored)
	}
	const double *bp[SR_NT];
#pragma unroll
	for (int nt = 0; nt < SR_NT; nt++) {
		const unsigned tile = eg * SR_NT + ((unsigned)nt < ntl ? (unsigned)nt : ntl - 1); // (tiles past the group: its last tile again, not stored)
		bp[nt] = S + ((size_t)tl.bl * Ec + (size_t)tile * SR_ET + li) * J + sg.joff;
	}

	sr_v4d acc[2][SR_NT];
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int nt = 0; nt < SR_NT; nt++) acc[rt][nt] = (sr_v4d){0, 0, 0, 0};
	double xx[2] = {0.0, 0.0};

	float a[2][4];
	sr_v4d b[SR_NT];
	// the four samples of this lane in block blk: columns 16 blk + 4 lk .. + 3 (the pad columns and what lies past the segment count as zero)
	auto request = [&](const unsigned blk) {
		const unsigned c = 16 * blk + 4 * lk;
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int q = 0; q < 4; q++) a[rt][q] = ap[rt][c + (unsigned)q < sg.len ? c + (unsigned)q : 0u];
		const unsigned cb = c < sg.plen ? c : 0u; // (plen and c are multiples of 4: the four columns are inside or outside together)
#pragma unroll
		for (int nt = 0; nt < SR_NT; nt++) b[nt] = *(const sr_v4d *)(bp[nt] + cb);
	};
	const unsigned nblk = (sg.plen + 15) / 16;
	request(0);
	for (unsigned blk = 0; blk < nblk; blk++) {
		const unsigned c = 16 * blk + 4 * lk;
		double ad[2][4];
		sr_v4d bd[SR_NT];
#pragma unroll
		for (int rt = 0; rt < 2; rt++)
#pragma unroll
			for (int q = 0; q < 4; q++) ad[rt][q] = c + (unsigned)q < sg.len ? (double)a[rt][q] : 0.0;
		const bool inb = c < sg.plen;
#pragma unroll
		for (int nt = 0; nt < SR_NT; nt++) bd[nt] = inb ? b[nt] : (sr_v4d){0, 0, 0, 0};
		if (blk + 1 < nblk) request(blk + 1); // (wave-uniform)
		if (first) {
#pragma unroll
			for (int rt = 0; rt < 2; rt++)
#pragma unroll
				for (int q = 0; q < 4; q++) xx[rt] = fma(ad[rt][q], ad[rt][q], xx[rt]);
		}
#pragma unroll
		for (int q = 0; q < 4; q++)
#pragma unroll
			for (int rt = 0; rt < 2; rt++)
#pragma unroll
				for (int nt = 0; nt < SR_NT; nt++) acc[rt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[rt][q], bd[nt][q], acc[rt][nt], 0, 0, 0);
	}

	// result register q of a tile: row 4 q + lk, column li (tools/probes/mfma_f64_layout.hip)
#pragma unroll
	for (int rt = 0; rt < 2; rt++)
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const unsigned r = (unsigned)rt * 16 + 4 * (unsigned)q + lk;
			if (r < count) {
				double *__restrict__ d = dots + ((tl.slot0 + r) * nseg + seg) * epad + e0 + (size_t)eg * SR_NT * SR_ET + li;
#pragma unroll
				for (int nt = 0; nt < SR_NT; nt++)
					if ((unsigned)nt < ntl) d[nt * SR_ET] = acc[rt][nt][q];
			}
		}
	if (first) {
#pragma unroll
		for (int rt = 0; rt < 2; rt++) {
			double v = xx[rt];
			v += __shfl_xor(v, 16, 64);
			v += __shfl_xor(v, 32, 64);
			const unsigned r = (unsigned)rt * 16 + li;
			if (lk == 0 && r < count) xxp[(tl.slot0 + r) * nseg + seg] = v;
		}
	}
}

__device__ __forceinline__ double sr_cc(const double *__restrict__ dots, const double *__restrict__ ss, unsigned s0, unsigned s1, unsigned nseg, unsigned epad,
                                        size_t slot, unsigned bl, unsigned e, double rx)
{
#pragma clang fp contract(off)
	double dot = 0.0, q = 0.0;
	for (unsigned s = s0; s < s1; s++) {
		dot += dots[(slot * nseg + s) * epad + e];
		q += ss[((size_t)bl * epad + e) * nseg + s];
	}
	return dot / rx / sqrt(q); // (rx = sqrt(sum c^2): the reference's similarity order; 0 / 0 = NaN for a dead row or a dead stretched reference)
}

// cc[(((b0 + bl) M + m) W + w) E + e] and fit[... 4] of every (row, window) of the round
__global__ void __launch_bounds__(256) k_sr_final(const double *__restrict__ dots, const double *__restrict__ xxp, const double *__restrict__ ss,
                                                  const unsigned *__restrict__ slot_of, const double *__restrict__ eps, unsigned E, unsigned epad, unsigned nseg,
                                                  unsigned W, unsigned seg0_0, unsigned seg0_1, unsigned seg0_2, unsigned seg0_3, unsigned seg0_4, size_t M,
                                                  unsigned b0, unsigned long long nitems, double *__restrict__ cc, double *__restrict__ fit)
{
#pragma clang fp contract(off)
	const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
	const unsigned long long item = (unsigned long long)blockIdx.x * 4 + wave;
	if (item >= nitems) return; // (the whole wave)
	const unsigned w = (unsigned)(item % W);
	const unsigned long long rw = item / W; // (ensemble of the round, m)
	const unsigned bl = (unsigned)(rw / M);
	const size_t o = ((size_t)b0 * M + rw) * W + w;
	const unsigned slot = slot_of[rw];
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	double *__restrict__ fo = fit + o * 4;
	if (slot == NOSLOT) { // the row does not take part
		if (cc) for (unsigned e = lane; e < E; e += 64) cc[o * E + e] = nan;
		if (lane == 0) { fo[0] = nan; fo[1] = nan; fo[2] = -1.0; fo[3] = 1.0; }
		return;
	}
	const unsigned s0 = w == 0 ? seg0_0 : w == 1 ? seg0_1 : w == 2 ? seg0_2 : seg0_3;
	const unsigned s1 = w == 0 ? seg0_1 : w == 1 ? seg0_2 : w == 2 ? seg0_3 : seg0_4;
	double xx = 0.0;
	for (unsigned s = s0; s < s1; s++) xx += xxp[(size_t)slot * nseg + s];
	const double rx = sqrt(xx);
	// the lane's own stretches in ascending order: the first largest; then across the lanes the largest, the smaller index on a tie
	double best = 0.0;
	unsigned bi = ~0u; // (none yet)
	for (unsigned e = lane; e < E; e += 64) {
		const double v = sr_cc(dots, ss, s0, s1, nseg, epad, slot, bl, e, rx);
		if (cc) cc[o * E + e] = v;
		if (v == v && (bi == ~0u || v > best)) { best = v; bi = e; }
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		const double ov = __shfl_xor(best, off, 64);
		const unsigned oi = (unsigned)__shfl_xor((int)bi, off, 64);
		if (oi != ~0u && (bi == ~0u || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
	}
	if (lane != 0) return;
	if (bi == ~0u) { fo[0] = nan; fo[1] = nan; fo[2] = -1.0; fo[3] = 1.0; return; }
	double eh = eps[bi], ch = best, edge = 1.0;
	if (bi > 0 && bi < E - 1) {
		const double cm = sr_cc(dots, ss, s0, s1, nseg, epad, slot, bl, bi - 1, rx), cp = sr_cc(dots, ss, s0, s1, nseg, epad, slot, bl, bi + 1, rx);
		const double den = cm - 2.0 * best + cp;
		if (den != 0.0) {
			const double d = 0.5 * (cm - cp) / den;
			eh = eps[bi] + d * (d >= 0.0 ? eps[bi + 1] - eps[bi] : eps[bi] - eps[bi - 1]);
			ch = best - 0.25 * (cm - cp) * d;
			edge = 0.0;
		}
	}
	fo[0] = eh; fo[1] = ch; fo[2] = (double)bi; fo[3] = edge;
}

extern "C" int tspws_stretch_grid(double *eps, double eps_max, unsigned E)
{
	if (!eps) return 1;
	if (E < 3 || E % 2 == 0 || !(eps_max > 0.0 && eps_max <= 0.5)) return 2;
	const double h = (double)((E - 1) / 2), step = eps_max / h;
	for (unsigned e = 0; e < E; e++) eps[e] = ((double)e - h) * step;
	return 0;
}

extern "C" int tspws_hip_stretch_rows(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                                      size_t ldr, double z, const double *h_eps, unsigned E, const size_t *h_win, unsigned W, double *d_cc, double *d_fit, void *s)
{
	// first what needs no plan
	if (!d_rows || !d_ref || !h_eps || !h_win || !d_fit) return fail(TSPWS_E_ARG, "stretch_rows: NULL");
	if (!E || E > SR_EMAX) return fail(TSPWS_E_ARG, "stretch_rows: 1 to 4096 stretch factors");
	if (const char *e = range_count_error(W, WINDOWS)) return refuse("stretch_rows", e);
	for (unsigned e = 0; e < E; e++) {
		if (!(fabs(h_eps[e]) <= 0.5)) return fail(TSPWS_E_ARG, "stretch_rows: a stretch factor that is NaN or outside [-0.5, 0.5]");
		if (e && !(h_eps[e] > h_eps[e - 1])) return fail(TSPWS_E_ARG, "stretch_rows: the stretch factors must increase strictly");
	}
	if (!std::isfinite(z)) return fail(TSPWS_E_ARG, "stretch_rows: a NaN or infinite zero-lag position");
	if (const char *e = range_empty_error(h_win, W, WINDOWS)) return refuse("stretch_rows", e);
	if (!pl) return fail(TSPWS_E_ARG, "stretch_rows: NULL");
	const size_t N = pl->N;
	if (ld < N) return fail(TSPWS_E_ARG, "stretch_rows: row stride below the trace length");
	if (ldr < N) return fail(TSPWS_E_ARG, "stretch_rows: reference row stride below the trace length");
	if (const char *e = range_past_error(h_win, W, N, WINDOWS)) return refuse("stretch_rows", e);
	if (!B || !M) return 0;
	if ((unsigned long long)B * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "stretch_rows: more than 2^32 rows");

	const SrCols cols = sr_columns(h_win, W);
	const unsigned nseg = (unsigned)cols.segs.size(), epad = sr_epad(E);
	const std::vector<size_t> nrows0 = participating_rows0(h_mtr, B, M);
	const std::vector<SrRound> rounds = sr_rounds(B, nrows0.data(), M, E, cols, tspws_part_budget_bytes());
	auto tab_of = [&](const SrRound &r) { return sr_tab(nseg, epad, sr_tiles(nrows0.data(), r.j0, r.j1), nrows0[r.j1] - nrows0[r.j0], (r.j1 - r.j0) * (size_t)M); };
	size_t max_tab = 0, max_part = 0, max_s = 0;
	for (const SrRound &r : rounds) {
		const size_t nb = r.j1 - r.j0, nt = sr_tiles(nrows0.data(), r.j0, r.j1);
		// one workgroup per 4 waves: the grids of the three launches
		const unsigned long long waves = std::max({(unsigned long long)nb * r.Ec * nseg, (unsigned long long)nt * ((r.Ec / SR_ET + SR_NT - 1) / SR_NT) * nseg,
		                                           (unsigned long long)nb * M * W});
		if ((waves + 3) / 4 > 0x7fffffffull) return fail(TSPWS_E_ARG, "stretch_rows: more than 2^33 waves in a round");
		max_tab = std::max(max_tab, tab_of(r).bytes);
		max_part = std::max(max_part, sr_part(nb, nrows0[r.j1] - nrows0[r.j0], nseg, epad).doubles * sizeof(double));
		max_s = std::max(max_s, sr_s_bytes(nb, r.Ec, cols.J));
	}

	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_stretch_stats &stats = pl->stretch_stats;
	stats = tspws_hip_stretch_stats();
	stats.segments = nseg;
	stats.rows = (unsigned)nrows0[B];
	stats.left_out = (unsigned)((size_t)B * M - nrows0[B]);
	BatchCall call(st);
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_SRP, std::max<size_t>(max_part, 16), &v))) return rc; // (the largest round's: the slots do not grow between rounds)
	double *part = (double *)v;
	if ((rc = scratch(pl, SCR_SRS, std::max<size_t>(max_s, 16), &v))) return rc;
	double *S = (double *)v;
	for (const SrRound &r : rounds) {
		const size_t nb = r.j1 - r.j0, nrows = nrows0[r.j1] - nrows0[r.j0], nt = sr_tiles(nrows0.data(), r.j0, r.j1);
		stats.rounds++;
		stats.chunks = std::max(stats.chunks, r.nchunks);
		const SrTab o = tab_of(r);
		char *blob = call.block(o.bytes), *tab;
		sr_fill_round(blob, o, r, M, h_mtr, cols, h_eps, E);
		if ((rc = call.upload(pl, SCR_SRTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const SrSeg *d_segs = (const SrSeg *)(tab + o.segs);
		const double *d_eps = (const double *)(tab + o.eps);
		const SrTile *d_tiles = (const SrTile *)(tab + o.tiles);
		const unsigned *d_list = (const unsigned *)(tab + o.list), *d_slot = (const unsigned *)(tab + o.slot_of);
		const SrPart p = sr_part(nb, nrows, nseg, epad);
		for (unsigned e0 = 0; e0 < epad; e0 += r.Ec) {
			const unsigned long long n1 = (unsigned long long)nb * r.Ec * nseg;
			hipLaunchKernelGGL(k_sr_stretch, dim3((unsigned)((n1 + 3) / 4)), dim3(256), 0, st, d_ref, ldr, (unsigned)N, z, d_segs, nseg, d_eps, E, epad, e0, r.Ec,
			                   (unsigned)r.j0, cols.J, n1, S, part + p.ss);
			if (!nt) continue; // (no row of the round takes part)
			const unsigned neg = (std::min(r.Ec, epad - e0) / SR_ET + SR_NT - 1) / SR_NT;
			const unsigned long long n2 = (unsigned long long)nt * neg * nseg;
			hipLaunchKernelGGL(k_sr_dots, dim3((unsigned)((n2 + 3) / 4)), dim3(256), 0, st, d_rows, ld, (size_t)M, d_segs, nseg, d_tiles, (unsigned)nt, d_list,
			                   (const double *)S, cols.J, e0, r.Ec, epad, neg, e0 == 0 ? 1 : 0, n2, part + p.dots, part + p.xx);
		}
		const unsigned long long n3 = (unsigned long long)nb * M * W;
		hipLaunchKernelGGL(k_sr_final, dim3((unsigned)((n3 + 3) / 4)), dim3(256), 0, st, (const double *)(part + p.dots), (const double *)(part + p.xx),
		                   (const double *)(part + p.ss), d_slot, d_eps, E, epad, nseg, W, cols.seg0[0], cols.seg0[1], cols.seg0[2], cols.seg0[3], cols.seg0[4],
		                   (size_t)M, (unsigned)r.j0, n3, d_cc, d_fit);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_stretch_rows_stats(const tspws_hip_plan *pl, tspws_hip_stretch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "stretch_rows_stats: NULL");
	*stats = pl->stretch_stats;
	return 0;
}
