// dtw_rows.hip -- dv/v by dynamic time warping (tspws_hip_dtw_rows; Hale 2013, Mikesell et al. 2015): per (row, lag range) the integer lag
// path lag[i] in [-Lmax, Lmax] that minimises the accumulated squared error between the normalised row and its normalised reference under the
// strain limit (the lag changes by at most one sample per b samples), and the regression of that path on the lag.  Rows are what the batched
// calls write ([B][M][ld] floats, [B][M] host counts).  The definition, operation by operation, is in include/tspws_hip.h; the device and the
// numpy checker (tests/dtw_rows_ref.py) agree bit for bit.
//
// The recurrence is sequential along the samples and parallel across the lags and the rows:
//   host     dtw_plan.h: lags per lane, samples and choice-plane words per range, rounds of whole ensembles inside TSPWS_PART_MB, per round
//            ONE table block (the slot of every row) and one upload
//   k_dtw<Q, b> one WAVE (one workgroup of 64) per (row of the round, range).  Lane j holds the Q consecutive lag indices j Q .. j Q + Q - 1, so of
//            the two neighbours of a lag at most one lies in another lane: two cross-lane moves per sample, as whole-wave shifts by one lane.
//            Forward.  The normalised row samples and the normalised reference reach of 64 samples are staged in LDS, the next chunk's floats
//            already on their way while this one is walked.  With V[i][l] = D[ib][l] + e[i-1][l] + .. + e[ib+1][l] (that order), the candidates
//            of lag l are D[i-1][l], V[i][l-1], V[i][l+1]: V is formed from a per-lane LDS ring of the last b D and b - 1 e and does not depend
//            on D[i-1] when b > 1, so the dependent chain of a sample is compare, select, add; b is a template parameter so that the ring's loads
//            of a sample are all issued before the first addition (one trip to the LDS, not b).  The choice goes into two bits; every 16 samples
//            a lane stores its Q words, coalesced, into the wave's plane in plan scratch.
//            Backward, the same wave.  The first smallest D[n-1][l] by a fixed reduction; then blocks of 8 words x nlp are loaded cooperatively
//            into LDS, lane 0 walks the block and leaves its 128 lags in LDS, and all lanes store them and add the integer sums.  Lane 0 the fit.
// Nothing is atomic, every output has one writer, and the values of (row, range) depend on that row, its reference, z, the range and the
// parameters alone: a repeated call is bit-identical, and batching, the other rows and ranges, the rounds and the padding change no bit.
#include "tspws_internal.h"
#include "batch_host.h"
#include "dtw_plan.h"

#include <climits>

struct DtwArgs { // the ranges of a call (dtw_plan.h: DtwGeom), by value
	unsigned n0[DT_WMAX], n[DT_WMAX], off[DT_WMAX + 1], words[DT_WMAX];
	unsigned long long poff[DT_WMAX + 1];
};

__device__ __forceinline__ long long dt_wave_sum(long long v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// v of the lane below (up = true: lane j takes lane j - 1's) or above, `edge` where there is none: the whole-wave shift by one lane of the
// data-parallel primitives (wave_shr:1 / wave_shl:1), two 32-bit moves on the vector pipe where __shfl_up / __shfl_down are four trips to the LDS
template <bool up>
__device__ __forceinline__ double dt_shift(double v, double edge)
{
	constexpr int ctrl = up ? 0x138 : 0x130;
	const int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), ctrl, 0xf, 0xf, false);
	const int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), ctrl, 0xf, 0xf, false);
	return __hiloint2double(hi, lo);
}

// max |x[k]|, k in [k0, k1), over the wave, in float (exact); *bad: a NaN among them
__device__ __forceinline__ float dt_absmax(const float *__restrict__ x, long long k0, long long k1, unsigned lane, bool *bad)
{
	float m = 0.0f;
	int nan = 0;
	for (long long k = k0 + lane; k < k1; k += 64) {
		const float v = x[k];
		nan |= v != v;
		m = fmaxf(m, fabsf(v));
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		m = fmaxf(m, __shfl_xor(m, o, 64));
		nan |= __shfl_xor(nan, o, 64);
	}
	*bad = nan != 0;
	return m;
}

template <int Q, int BB>
__global__ void __launch_bounds__(64) k_dtw(const float *__restrict__ rows, size_t ld, const float *__restrict__ ref, size_t ldr, unsigned N, size_t M, unsigned W,
                                            unsigned Lmax, double z, const DtwArgs a, const unsigned *__restrict__ slot_of, size_t row0, unsigned ringD_o,
                                            unsigned ringE_o, unsigned stage_o, unsigned stage_doubles, unsigned *__restrict__ planes, int *__restrict__ d_lag,
                                            double *__restrict__ d_fit)
{
#pragma clang fp contract(off) // every operation of the definition is rounded on its own
	extern __shared__ __attribute__((aligned(16))) char lds[];
	constexpr unsigned NLP = 64 * Q;
	constexpr int NR = Q == 1 ? 2 : Q == 2 ? 3 : 5; // floats of the reference reach per lane and chunk: 64 + 2 Lmax <= 64 NR
	constexpr unsigned b = BB; // the strain limit
	const unsigned lane = threadIdx.x;
	const unsigned w = blockIdx.x % W;
	const size_t rw = blockIdx.x / W;                // row of the round
	const size_t row = row0 + rw;                    // b M + m
	const unsigned slot = slot_of[rw];
	const unsigned n0 = a.n0[w], nw = a.n[w], nl = 2 * Lmax + 1, T = a.off[DT_WMAX];
	const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
	double *__restrict__ fo = d_fit + (row * W + w) * 6;
	int *__restrict__ lo = d_lag ? d_lag + row * T + a.off[w] : nullptr;

	const float *__restrict__ cp = rows + row * ld;
	const float *__restrict__ rp = ref + (row / M) * ldr;
	bool dead = slot == NOSLOT;
	double ac = 0.0, ar = 0.0;
	if (!dead) { // (wave-uniform)
		bool badc, badr;
		const long long k0 = (long long)n0 - Lmax < 0 ? 0 : (long long)n0 - Lmax, k1 = (long long)n0 + nw + Lmax > (long long)N ? (long long)N : (long long)n0 + nw + Lmax;
		const float mc = dt_absmax(cp, n0, (long long)n0 + nw, lane, &badc), mr = dt_absmax(rp, k0, k1, lane, &badr);
		dead = badc || badr || !(mc > 0.0f) || !(mr > 0.0f) || mc == __int_as_float(0x7f800000) || mr == __int_as_float(0x7f800000);
		ac = 1.0 / (double)mc;
		ar = 1.0 / (double)mr;
	}
	if (dead) { // the row does not take part, or the (row, range) is dead
		if (lo) for (unsigned i = lane; i < nw; i += 64) lo[i] = INT_MIN;
		if (lane == 0) { fo[0] = nan; fo[1] = nan; fo[2] = nan; fo[3] = nan; fo[4] = nan; fo[5] = -1.0; }
		return;
	}

	unsigned *__restrict__ plane = planes + (size_t)slot * a.poff[DT_WMAX] + a.poff[w];
	double *ringD = (double *)(lds + ringD_o), *ringE = (double *)(lds + ringE_o), *stage = (double *)(lds + stage_o);

	// ---- forward ----
	// a chunk's floats: sample n0 + i0 + lane of the row, samples clamp(n0 + i0 + t - Lmax, 0, N - 1), t = lane + 64 k, of the reference
	float pc, pr[NR];
	auto request = [&](const unsigned i0) {
		pc = i0 + lane < nw ? cp[n0 + i0 + lane] : 0.0f;
#pragma unroll
		for (int k = 0; k < NR; k++) {
			long long s = (long long)n0 + i0 + lane + 64 * k - Lmax;
			s = s < 0 ? 0 : s > (long long)N - 1 ? (long long)N - 1 : s;
			pr[k] = rp[s];
		}
	};
	auto deposit = [&](double *buf) { // buf: [64] row | [64 + 64 Q] reference
		buf[lane] = (double)pc * ac;
#pragma unroll
		for (int k = 0; k < NR; k++)
			if (lane + 64 * k < DT_CHUNK + NLP) buf[DT_CHUNK + lane + 64 * k] = (double)pr[k] * ar;
	};

	double D[Q];
	unsigned bits[Q];
#pragma unroll
	for (int q = 0; q < Q; q++) { D[q] = 0.0; bits[q] = 0; }
	unsigned sd = 0, se = 0; // i % b, i % (b - 1)
	request(0);
	for (unsigned i = 0; i < nw; i++) {
		const unsigned ii = i & (DT_CHUNK - 1);
		const double *buf = stage + ((i / DT_CHUNK) & 1) * stage_doubles;
		if (ii == 0) { // (wave-uniform)
			deposit(const_cast<double *>(buf));
			__syncthreads();
			if (i + DT_CHUNK < nw) request(i + DT_CHUNK);
		}
		const double cn = buf[ii];
		double e[Q];
#pragma unroll
		for (int q = 0; q < Q; q++) {
			const double d = cn - buf[DT_CHUNK + ii + lane * Q + q];
			e[q] = lane * Q + q < nl ? d * d : 0.0;
		}
		if (i == 0) {
#pragma unroll
			for (int q = 0; q < Q; q++) D[q] = lane * Q + q < nl ? e[q] : inf;
		} else {
			double V[Q];
			if constexpr (BB == 1) {
#pragma unroll
				for (int q = 0; q < Q; q++) V[q] = D[q];
			} else {
				const unsigned sb = i >= b ? sd : 0; // D[ib]: i - b sits where D[i] will go
#pragma unroll
				for (int q = 0; q < Q; q++) V[q] = ringD[(sb * Q + q) * 64 + lane];
				if (i >= b) { // (wave-uniform) e[i-1] .. e[i-b+1]: every load issued before the first addition
					double ev[BB - 1][Q];
#pragma unroll
					for (int c = 0; c < BB - 1; c++) {
						const unsigned s = se >= (unsigned)c + 1 ? se - 1 - c : se + (BB - 1) - 1 - c;
#pragma unroll
						for (int q = 0; q < Q; q++) ev[c][q] = ringE[(s * Q + q) * 64 + lane];
					}
#pragma unroll
					for (int c = 0; c < BB - 1; c++)
#pragma unroll
						for (int q = 0; q < Q; q++) V[q] = V[q] + ev[c][q];
				} else { // the first b samples: e[i-1] .. e[1]
					unsigned s = se;
					for (unsigned c = 0; c + 1 < i; c++) {
						s = s ? s - 1 : b - 2;
#pragma unroll
						for (int q = 0; q < Q; q++) V[q] = V[q] + ringE[(s * Q + q) * 64 + lane];
					}
				}
			}
			const double up = dt_shift<true>(V[Q - 1], inf), dn = dt_shift<false>(V[0], inf);
			const unsigned sh = 2 * (i & 15);
#pragma unroll
			for (int q = 0; q < Q; q++) {
				const double dc = D[q];
				const double dm = q > 0 ? V[q > 0 ? q - 1 : 0] : up; // (lane 0 has no lane below: +inf)
				const double dp = q < Q - 1 ? V[q < Q - 1 ? q + 1 : 0] : dn; // (the index after the last lag is a pad index: +inf)
				unsigned ch;
				double best;
				if (dc <= dm && dc <= dp) { ch = 0; best = dc; }
				else if (dm <= dp) { ch = 1; best = dm; }
				else { ch = 2; best = dp; }
				D[q] = lane * Q + q < nl ? e[q] + best : inf; // (a pad index stays at +inf: it is the missing neighbour of the last lag)
				bits[q] |= ch << sh;
			}
		}
		if constexpr (BB > 1) {
#pragma unroll
			for (int q = 0; q < Q; q++) {
				ringD[(sd * Q + q) * 64 + lane] = D[q];
				ringE[(se * Q + q) * 64 + lane] = e[q];
			}
			sd = sd + 1 == b ? 0 : sd + 1;
			se = se + 1 >= b - 1 ? 0 : se + 1;
		}
		if ((i & 15) == 15 || i == nw - 1) {
			unsigned *p = plane + (size_t)(i >> 4) * NLP + lane * Q;
#pragma unroll
			for (int q = 0; q < Q; q++) { p[q] = bits[q]; bits[q] = 0; }
		}
	}

	// ---- the first smallest D[n-1][l] ----
	double best = inf;
	unsigned bi = ~0u;
#pragma unroll
	for (int q = 0; q < Q; q++)
		if (lane * Q + q < nl && (bi == ~0u || D[q] < best)) { best = D[q]; bi = lane * Q + q; }
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const double ov = __shfl_xor(best, o, 64);
		const unsigned oi = (unsigned)__shfl_xor((int)bi, o, 64);
		if (oi != ~0u && (bi == ~0u || ov < best || (ov == best && oi < bi))) { best = ov; bi = oi; }
	}

	// ---- backward ----
	__threadfence(); // the plane's words, stored by all lanes, are read by all lanes
	__syncthreads(); // (the rings are done: the block of words and the lags lie over them)
	unsigned *bw = (unsigned *)lds;
	int *bl = (int *)(lds + DT_BACK * NLP * 4);
	const unsigned nwords = a.words[w];
	int l = (int)bi - (int)Lmax;       // lane 0's walk: the lag at sample i
	unsigned hold = 0;                 // samples below i whose lag a slanted choice has fixed already
	long long Sl = 0, Sil = 0, Sll = 0, clip = 0;
	if (lane == 0) {
		if (lo) lo[nw - 1] = l;
		Sl = l; Sil = (long long)(nw - 1) * l; Sll = (long long)l * l; clip = (unsigned)(l < 0 ? -l : l) == Lmax;
	}
	for (unsigned wb = (nwords + DT_BACK - 1) / DT_BACK; wb-- > 0;) {
		const unsigned w0 = wb * DT_BACK, cntw = nwords - w0 < DT_BACK ? nwords - w0 : DT_BACK;
		for (unsigned k = lane; k < cntw * NLP; k += 64) bw[k] = plane[(size_t)w0 * NLP + k];
		__syncthreads();
		const unsigned ilo = 16 * w0 > 1 ? 16 * w0 : 1, ihi = 16 * (w0 + cntw) - 1 < nw - 1 ? 16 * (w0 + cntw) - 1 : nw - 1; // samples i of the block with a choice
		if (lane == 0) {
			for (unsigned i = ihi + 1; i-- > ilo;) { // sets lag[i - 1]
				if (hold) hold--;
				else {
					const unsigned ch = (bw[((i >> 4) - w0) * NLP + (unsigned)(l + (int)Lmax)] >> (2 * (i & 15))) & 3u;
					if (ch) {
						l += ch == 1 ? -1 : 1;
						hold = (i < b ? i : b) - 1; // lag[i-1] .. lag[ib] are l: one set here
					}
				}
				bl[i - 16 * w0] = l;
			}
		}
		__syncthreads();
		for (unsigned k = lane; k < 16 * cntw; k += 64) {
			const unsigned i = 16 * w0 + k;
			if (i >= ilo && i <= ihi) {
				const int v = bl[k];
				if (lo) lo[i - 1] = v;
				Sl += v; Sil += (long long)(i - 1) * v; Sll += (long long)v * v; clip += (unsigned)(v < 0 ? -v : v) == Lmax;
			}
		}
		__syncthreads();
	}
	Sl = dt_wave_sum(Sl); Sil = dt_wave_sum(Sil); Sll = dt_wave_sum(Sll); clip = dt_wave_sum(clip);
	if (lane != 0) return;

	// ---- the fit ----
	const long long n = nw;
	const double S = (double)n, Si = (double)(n * (n - 1) / 2), Sii = (double)((n - 1) * n * (2 * n - 1) / 6);
	const double dSl = (double)Sl, dSil = (double)Sil, dSll = (double)Sll;
	const double den = S * Sii - Si * Si;
	const double num = S * dSil - Si * dSl;
	const double eh = num / den;
	const double t0 = ((double)n0 - z) + Si / S;
	const double ic = dSl / S - eh * t0;
	const double res = (dSll - (dSl / S) * dSl) - eh * (num / S);
	const double rms = sqrt((res > 0.0 ? res : 0.0) / S);
	const double err = rms * sqrt(S / den);
	fo[0] = eh; fo[1] = ic; fo[2] = err; fo[3] = rms; fo[4] = best / S; fo[5] = (double)clip;
}

typedef void (*DtwKernel)(const float *, size_t, const float *, size_t, unsigned, size_t, unsigned, unsigned, double, const DtwArgs, const unsigned *, size_t, unsigned,
                          unsigned, unsigned, unsigned, unsigned *, int *, double *);
// the instantiation for Q lags per lane and the strain limit b
static DtwKernel dt_kernel(unsigned Q, unsigned b)
{
#define DT_ROW(Q) {k_dtw<Q, 1>, k_dtw<Q, 2>, k_dtw<Q, 3>, k_dtw<Q, 4>, k_dtw<Q, 5>, k_dtw<Q, 6>, k_dtw<Q, 7>, k_dtw<Q, 8>}
	static const DtwKernel tab[3][DT_BMAX] = {DT_ROW(1), DT_ROW(2), DT_ROW(4)};
#undef DT_ROW
	return tab[Q == 1 ? 0 : Q == 2 ? 1 : 2][b - 1];
}

extern "C" int tspws_hip_dtw_rows(tspws_hip_plan *pl, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref, size_t ldr,
                                  double z, const tspws_dtw_par *par, const size_t *h_win, unsigned W, int *d_lag, double *d_fit, void *s)
{
	// first what needs no plan
	if (!d_rows || !d_ref || !par || !h_win || !d_fit) return fail(TSPWS_E_ARG, "dtw_rows: NULL");
	const DtwPar P = {par->Lmax, par->b};
	if (const char *e = dt_par_error(P)) return refuse("dtw_rows", e);
	if (const char *e = dt_range_error(h_win, W)) return refuse("dtw_rows", e);
	if (!std::isfinite(z)) return fail(TSPWS_E_ARG, "dtw_rows: a NaN or infinite zero-lag position");
	if (!pl) return fail(TSPWS_E_ARG, "dtw_rows: NULL");
	const size_t N = pl->N;
	if (ld < N) return fail(TSPWS_E_ARG, "dtw_rows: row stride below the trace length");
	if (ldr < N) return fail(TSPWS_E_ARG, "dtw_rows: reference row stride below the trace length");
	if (const char *e = range_past_error(h_win, W, N, LAG_RANGES)) return refuse("dtw_rows", e);
	if (!B || !M) return 0;
	if ((unsigned long long)B * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, "dtw_rows: more than 2^32 - 16 rows");

	const DtwGeom g = dt_geom(P, h_win, W);
	const DtwLds lds = dt_lds(P, g.Q);
	const std::vector<size_t> nrows0 = participating_rows0(h_mtr, B, M);
	const std::vector<Round> rounds = dt_rounds(B, nrows0.data(), M, g, tspws_part_budget_bytes());
	size_t max_tab = 0, max_planes = 0;
	for (const Round &r : rounds) {
		if ((unsigned long long)(r.j1 - r.j0) * M * W > 0x7fffffffull) return fail(TSPWS_E_ARG, "dtw_rows: more than 2^31 waves in a round");
		max_tab = std::max(max_tab, dt_tab((r.j1 - r.j0) * (size_t)M).bytes);
		max_planes = std::max(max_planes, dt_plane_bytes(nrows0[r.j1] - nrows0[r.j0], g));
	}
	DtwArgs a;
	for (unsigned w = 0; w < DT_WMAX; w++) { a.n0[w] = g.n0[w]; a.n[w] = g.n[w]; a.words[w] = g.words[w]; }
	for (unsigned w = 0; w <= DT_WMAX; w++) { a.off[w] = g.off[w]; a.poff[w] = g.poff[w]; }

	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	tspws_hip_dtw_stats &stats = pl->dtw_stats;
	stats = tspws_hip_dtw_stats();
	stats.rows = (unsigned)nrows0[B];
	stats.left_out = (unsigned)((size_t)B * M - nrows0[B]);
	stats.lags = g.nl;
	stats.samples = g.T();
	BatchCall call(st);
	int rc;
	void *v;
	if ((rc = scratch(pl, SCR_DTP, std::max<size_t>(max_planes, 16), &v))) return rc; // (the largest round's: the slot does not grow between rounds)
	unsigned *planes = (unsigned *)v;
	for (const Round &r : rounds) {
		const size_t nb = r.j1 - r.j0;
		stats.rounds++;
		const DtwTab o = dt_tab(nb * M);
		char *blob = call.block(o.bytes), *tab;
		dt_fill_round(blob, o, r, M, h_mtr);
		if ((rc = call.upload(pl, SCR_DTTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const unsigned *d_slot = (const unsigned *)(tab + o.slot_of);
		const dim3 grid((unsigned)(nb * M * W)), block(64);
		hipLaunchKernelGGL(dt_kernel(g.Q, P.b), grid, block, lds.bytes, st, d_rows, ld, d_ref, ldr, (unsigned)N, (size_t)M, W, P.Lmax, z, a, d_slot, r.j0 * (size_t)M,
		                   lds.ringD, lds.ringE, lds.stage, lds.stage_doubles, planes, d_lag, d_fit);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_dtw_rows_stats(const tspws_hip_plan *pl, tspws_hip_dtw_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "dtw_rows_stats: NULL");
	*stats = pl->dtw_stats;
	return 0;
}
