// batch_kernels.h -- small kernels that the batched entry points share: the gather of batch.hip and jk_batch.hip, the class time sums and the
// replicas' finish (weighted sets, linear stacks) of jk_single.hip and jk_batch.hip, the per-row weight mode of those and of the row batches,
// the rows' finish (weighted sets, float epilogue) of the row batches (sub_batch.hip, boot_batch.hip; the epilogue also of weighted_batch.hip),
// whose own kernels -- the accumulation and the linear stack, templates over the row's code -- are in row_batch.h.  Every unit that includes
// this header gets its own copy (internal linkage: the units are compiled without relocatable device code).
#pragma once

#include "tspws_internal.h"

// slot j of a gathered batch = trace src[j] of x (row stride ld); src[j] < 0: an idle lane of an ensemble's last block (zeros)
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_batch_gather(const float *__restrict__ x, size_t ld, const long long *__restrict__ src, unsigned N,
                                                             float *__restrict__ xg)
{
	const unsigned n = blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const long long t = src[blockIdx.y];
	xg[(size_t)blockIdx.y * N + n] = t >= 0 ? x[(size_t)t * ld + n] : 0.f;
}

// FP64 time-domain sum of every class (blockIdx.y): T[k][n] = sum over its traces in trace order of (double) x[i][n]
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_j1_time(const float *__restrict__ x, size_t ld, size_t N, const unsigned *__restrict__ idx,
                                                        const unsigned *__restrict__ cptr, double *__restrict__ T)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned q1 = cptr[blockIdx.y + 1];
	double acc = 0;
	for (unsigned q0 = cptr[blockIdx.y]; q0 < q1; q0 += 8) { // eight rows' loads in flight
		float v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = q0 + (unsigned)j < q1 ? x[(size_t)idx[q0 + j] * ld + n] : 0.f;
#pragma unroll
		for (int j = 0; j < 8; j++) if (q0 + (unsigned)j < q1) acc += (double)v[j];
	}
	T[(size_t)blockIdx.y * N + n] = acc;
}

__device__ __forceinline__ int j1_weight_mode(double wu, int unbiased, unsigned K) // tspws_weight_mode (inverse.hip), per replica
{
	if (wu == 2 && unbiased && K != 1) return 3;
	if (wu == 2) return 0;
	if (wu == 1) return 1;
	return 2;
}

// One ensemble of a round to the replicas' finish below.  (jk_single.hip: ONE descriptor, everything but ncls zero, and no main rows.)
struct JbEns { unsigned cls0, ncls, kept_off, kc_off, M, row; }; // classes [cls0, cls0 + ncls) of the round, kept[C][ncls] / K_c[C] offsets, traces, output row

constexpr unsigned JB_NT = 64;      // coefficients per workgroup of k_jb_finish
constexpr unsigned JB_RPB = 8;      // rows per workgroup
constexpr unsigned JB_LDS_MAX = 24; // classes the LDS form holds (2 KB each: <= 48 KB of the CU's 160 KB, three workgroups resident)

// Weighted coefficients of rows q0 + y, y < nq, of ensemble blockIdx.z of the round.  Rows of an ensemble: with `main`, row 0 = OUT and row 1 =
// ST of the plain stack (all classes, K = M = M_b); then replica c = q - 2 main: ST_c / PS_c = sums of the kept classes' planes in class
// order, OUT = ST_c * weight(PS_c; K = M = K_c).  One thread per coefficient (consecutive double2: coalesced),
// RPB rows per workgroup; LDS: the coefficient's class values are staged once (each thread reads back only its own entries: no barrier).
template <bool LDS>
[[maybe_unused]] static __global__ void __launch_bounds__(JB_NT) k_jb_finish(const double2 *__restrict__ planes, size_t ncoef, const JbEns *__restrict__ ens,
                                                     const char *__restrict__ kept, const unsigned *__restrict__ Kc, unsigned main, unsigned q0, unsigned nq,
                                                     double wu, int unbiased, double2 *__restrict__ OUT)
{
	extern __shared__ double2 jb_sh[]; // [class][ST | PS][JB_NT]
	const size_t i = (size_t)blockIdx.x * JB_NT + threadIdx.x;
	if (i >= ncoef) return;
	const JbEns e = ens[blockIdx.z];
	const double2 *pl = planes + (size_t)e.cls0 * 2 * ncoef;
	if (LDS)
		for (unsigned k = 0; k < e.ncls; k++) {
			jb_sh[(2 * k) * JB_NT + threadIdx.x] = pl[(size_t)k * 2 * ncoef + i];
			jb_sh[(2 * k + 1) * JB_NT + threadIdx.x] = pl[(size_t)k * 2 * ncoef + ncoef + i];
		}
	const unsigned y1 = min(nq, (blockIdx.y + 1) * JB_RPB);
	for (unsigned y = blockIdx.y * JB_RPB; y < y1; y++) {
		const unsigned q = q0 + y;
		const bool all = q < 2 * main;
		const char *kr = kept + e.kept_off + (size_t)(all ? 0 : q - 2 * main) * e.ncls;
		double2 st = make_double2(0, 0), ps = make_double2(0, 0);
		for (unsigned k = 0; k < e.ncls; k++) {
			if (!all && !kr[k]) continue; // (wave-uniform)
			const double2 a = LDS ? jb_sh[(2 * k) * JB_NT + threadIdx.x] : pl[(size_t)k * 2 * ncoef + i];
			const double2 b = LDS ? jb_sh[(2 * k + 1) * JB_NT + threadIdx.x] : pl[(size_t)k * 2 * ncoef + ncoef + i];
			st.x += a.x; st.y += a.y; ps.x += b.x; ps.y += b.y;
		}
		double2 o;
		if (all) o = q == 0 ? weight_value(st, ps, j1_weight_mode(wu, unbiased, e.M), (double)e.M, (double)e.M, wu) : st;
		else {
			const unsigned K = Kc[e.kc_off + q - 2 * main];
			o = K ? weight_value(st, ps, j1_weight_mode(wu, unbiased, K), (double)K, (double)K, wu) : make_double2(0, 0);
		}
		OUT[((size_t)blockIdx.z * nq + y) * ncoef + i] = o;
	}
}

// linear stacks of replicas c0 + blockIdx.y of ensemble blockIdx.z: (float)((sum of the kept classes' time sums) * (1 / K_c)), the
// two-stage jackknife's time-domain formula (ts_pws1f_lib.c:799-811) with every trace its own group
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_jb_linear(const double *__restrict__ T, size_t N, const JbEns *__restrict__ ens, const char *__restrict__ kept,
                                                   const unsigned *__restrict__ Kc, unsigned C, unsigned c0, float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const JbEns e = ens[blockIdx.z];
	const unsigned c = c0 + blockIdx.y, K = Kc[e.kc_off + c];
	const char *kr = kept + e.kept_off + (size_t)c * e.ncls;
	double acc = 0;
	for (unsigned k = 0; k < e.ncls; k++) if (kr[k]) acc += T[(size_t)(e.cls0 + k) * N + n];
	out[((size_t)e.row * C + c) * N + n] = K ? (float)(acc * (1.0 / (double)K)) : 0.f;
}

// A single-stage ensemble of a round of row_batch.h: first trace, its codes in the round's table, traces, index of its first trace in the
// round's partials, output block.  The codes of group g of 8 rows hold one entry per trace j at [bits_off + g m + j]: sub_batch.hip a byte
// with the 8 mask bits, boot_batch.hip an aligned 8-byte word with the 8 count bytes, weighted_batch.hip an aligned 64-byte block with the
// 8 FP64 weights.
struct SbEns { unsigned long long t0, bits_off; unsigned m, part0, row, pad; };

// weighted coefficients of the rows r0 + blockIdx.y of the round: OUT = ST * weight(PS; K = M = K_r), the mode by the row's own K (K = 1: the
// K = 1 rule, ts_pws1f_lib.c:972); K = 0: a zero set
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_sb_weight(double2 *__restrict__ OUT, const double2 *__restrict__ planes, size_t ncoef,
                                                                            const unsigned *__restrict__ Kc, size_t r0, double wu, int unbiased)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= ncoef) return;
	const size_t r = r0 + blockIdx.y;
	const unsigned K = Kc[r];
	double2 o = make_double2(0, 0);
	if (K) o = weight_value(planes[r * 2 * ncoef + i], planes[r * 2 * ncoef + ncoef + i], j1_weight_mode(wu, unbiased, K), (double)K, (double)K, wu);
	OUT[(size_t)blockIdx.y * ncoef + i] = o;
}

// tsPWS_out of the rows r0 + blockIdx.y of the round (row r = mask r % M of the round's ensemble r / M): (float) x to block [b][m]; K = 0: zero
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_sb_epilogue(const double *__restrict__ x, size_t N, const SbEns *__restrict__ ens,
                                                                              const unsigned *__restrict__ Kc, unsigned M, size_t r0, float *__restrict__ ts_out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const size_t r = r0 + blockIdx.y;
	const unsigned q = (unsigned)(r % M);
	ts_out[((size_t)ens[r / M].row * M + q) * N + n] = Kc[r] ? (float)x[(size_t)blockIdx.y * N + n] : 0.f;
}
