// batch_kernels.h -- small kernels that the batched entry points share (batch.hip, jk_single.hip, jk_batch.hip).  Every unit that includes
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
