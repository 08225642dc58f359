// jk_single.hip -- single-stage jackknife: delete-d replicas from per-class stacks.
// Reference citations are relative to /root/reference/src.
//
// The reference implements the jackknife for two-stage stacks only; its single-stage variant is an empty stub (ts_pws1f_lib.c:711-716).
// This unit fills that gap with the single-stage resampling body (tspws_subsmpl_float, :501-610) applied to every replica's mask, K
// replaced by the replica's trace count K_c.  The linear and phase stacks are plain sums over traces, and a delete-d replica is a union
// of day-of-year bins, so every replica is a sum of per-CLASS stacks (a class = the traces whose selection columns are identical):
//   class pass   every trace is transformed ONCE (tspws_forward_parts) and added to the ST / PS plane pair of its class
//                (k_j1_accumulate, the traces of a class in trace order); the FP64 time-domain class sums feed the linear stacks
//                (k_j1_time).  The FP64-bound work does not grow with the replica count C.
//   finish       per batch of replicas: ST_c / PS_c as sums of the kept classes' planes and the weighted coefficients with each
//                replica's own K_c (k_j1_finish: a coefficient's class values are staged once in LDS for RPB replicas), the batched
//                inverse, the float epilogue; ls_c from the class time sums (k_j1_linear).
// FP64 summation order: by class, then over the kept classes in class order (not trace order); the float outputs agree with a
// trace-order restatement to the last bits.  A replica without traces (K_c = 0) gets zero rows and count 0.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include <string>
#include <unordered_map>

#define is_two_stage tspws_is_two_stage

// ------------------------------------------------------------------------------------------
// host: classes of a selection
// ------------------------------------------------------------------------------------------
extern "C" int tspws_selection_classes(const char *sel, unsigned C, size_t mtr, unsigned *class_of_trace, char *kept, unsigned *ncls)
{
	if (!sel || !class_of_trace || !ncls) return fail(TSPWS_E_ARG, "selection_classes: NULL");
	const size_t nbytes = ((size_t)C + 7) / 8;
	std::unordered_map<std::string, unsigned> id;
	std::vector<size_t> first; // first trace of every class
	std::string key(nbytes, '\0');
	for (size_t i = 0; i < mtr; i++) {
		std::fill(key.begin(), key.end(), '\0');
		for (unsigned c = 0; c < C; c++)
			if (sel[(size_t)c * mtr + i] == 1) key[c >> 3] = (char)(key[c >> 3] | (1 << (c & 7)));
		auto it = id.find(key);
		if (it == id.end()) { it = id.emplace(key, (unsigned)first.size()).first; first.push_back(i); }
		class_of_trace[i] = it->second;
	}
	const unsigned n = (unsigned)first.size();
	if (kept)
		for (unsigned c = 0; c < C; c++)
			for (unsigned k = 0; k < n; k++) kept[(size_t)c * n + k] = sel[(size_t)c * mtr + first[k]] == 1 ? 1 : 0;
	*ncls = n;
	return 0;
}

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// ST_k += Y_b, PS_k += Y_b/|Y_b| over the traces b of class k = blockIdx.y in this batch (rg[k] = their range in idx, global trace
// indices, ascending); one thread per coefficient: a class plane pair is read and written once per batch, every transformed trace
// is read once.  Planes: [class][ST | PS], 2 ncoef apart.
__global__ void __launch_bounds__(256) k_j1_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                       size_t ncoef, const uint2 *__restrict__ rg, const unsigned *__restrict__ idx, size_t t0,
                                                       double2 *__restrict__ planes)
{
	const uint2 r = rg[blockIdx.y];
	if (r.x == r.y) return;
	unsigned lo = 0, hi = S;
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (sc[mid].acc_off <= blockIdx.x) lo = mid; else hi = mid;
	}
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	const unsigned k = (blockIdx.x - sc[lo].acc_off) * 256 + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const double2 *p0 = part + sc[lo].part_off + k;
	double2 *ST = planes + (size_t)blockIdx.y * 2 * ncoef, *PS = ST + ncoef;
	double2 st = ST[i], ps = PS[i];
	for (unsigned q0 = r.x; q0 < r.y; q0 += 4) { // four traces' loads in flight, the additions in trace order
		double2 a[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			a[j] = make_double2(0, 0);
			if (q0 + (unsigned)j < r.y) a[j] = p0[(size_t)(idx[q0 + j] - t0) * npart];
		}
		for (unsigned sp = 1; sp < nsplit; sp++) {
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (q0 + (unsigned)j < r.y) { const double2 t = p0[(size_t)(idx[q0 + j] - t0) * npart + (size_t)sp * Ns]; a[j].x += t.x; a[j].y += t.y; }
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (q0 + (unsigned)j < r.y) { st.x += a[j].x; st.y += a[j].y; add_unit_phasor(ps, a[j]); }
	}
	ST[i] = st;
	PS[i] = ps;
}

static constexpr unsigned J1_NT = 64;      // coefficients per workgroup of k_j1_finish
static constexpr unsigned J1_RPB = 8;      // replicas per workgroup
static constexpr unsigned J1_LDS_MAX = 24; // classes the LDS form holds (2 KB each: <= 48 KB)

// Weighted coefficients of replicas c0 + j, j < nr: ST_c / PS_c = sums of the planes of the classes the replica keeps (class order),
// OUT[j] = ST_c * weight(PS_c; K = M = K_c).  One thread per coefficient, RPB replicas per workgroup (grid.y); LDS: the coefficient's
// class values are staged once (each thread reads back only its own entries: no barrier) instead of re-read per replica.
template <bool LDS>
__global__ void __launch_bounds__(J1_NT) k_j1_finish(const double2 *__restrict__ planes, unsigned ncls, size_t ncoef, const char *__restrict__ kept,
                                                     const unsigned *__restrict__ Kc, unsigned c0, unsigned nr, double wu, int unbiased,
                                                     double2 *__restrict__ OUT)
{
	extern __shared__ double2 j1_sh[]; // [class][ST | PS][J1_NT]
	const size_t i = (size_t)blockIdx.x * J1_NT + threadIdx.x;
	if (i >= ncoef) return;
	if (LDS)
		for (unsigned k = 0; k < ncls; k++) {
			j1_sh[(2 * k) * J1_NT + threadIdx.x] = planes[(size_t)k * 2 * ncoef + i];
			j1_sh[(2 * k + 1) * J1_NT + threadIdx.x] = planes[(size_t)k * 2 * ncoef + ncoef + i];
		}
	const unsigned j1 = min(nr, (blockIdx.y + 1) * J1_RPB);
	for (unsigned j = blockIdx.y * J1_RPB; j < j1; j++) {
		const unsigned c = c0 + j, K = Kc[c];
		const char *kr = kept + (size_t)c * ncls;
		double2 st = make_double2(0, 0), ps = make_double2(0, 0);
		for (unsigned k = 0; k < ncls; k++) {
			if (!kr[k]) continue; // (wave-uniform)
			const double2 a = LDS ? j1_sh[(2 * k) * J1_NT + threadIdx.x] : planes[(size_t)k * 2 * ncoef + i];
			const double2 b = LDS ? j1_sh[(2 * k + 1) * J1_NT + threadIdx.x] : planes[(size_t)k * 2 * ncoef + ncoef + i];
			st.x += a.x; st.y += a.y; ps.x += b.x; ps.y += b.y;
		}
		OUT[(size_t)j * ncoef + i] = K ? weight_value(st, ps, j1_weight_mode(wu, unbiased, K), (double)K, (double)K, wu) : make_double2(0, 0);
	}
}

// linear stacks of replicas c0 + blockIdx.y: (float)((sum of the kept classes' time sums) * (1 / K_c)), the two-stage jackknife's
// time-domain formula (:799-811) with every trace its own group
__global__ void __launch_bounds__(256) k_j1_linear(const double *__restrict__ T, size_t N, unsigned ncls, const char *__restrict__ kept,
                                                   const unsigned *__restrict__ Kc, unsigned c0, float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned c = c0 + blockIdx.y, K = Kc[c];
	const char *kr = kept + (size_t)c * ncls;
	double acc = 0;
	for (unsigned k = 0; k < ncls; k++) if (kr[k]) acc += T[(size_t)k * N + n];
	out[(size_t)c * N + n] = K ? (float)(acc * (1.0 / (double)K)) : 0.f;
}

// ------------------------------------------------------------------------------------------
// the call
// ------------------------------------------------------------------------------------------
extern "C" int tspws_hip_jackknife_single(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t mtr, const char *h_sel,
                                          unsigned C, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *s)
{
	if (!pl || !p || !h_sel || !d_ls_out || !d_ts_out || !h_mtr_out || (!d_x && mtr)) return fail(TSPWS_E_ARG, "jackknife_single: NULL");
	if (is_two_stage(p, mtr)) return fail(TSPWS_E_ARG, "jackknife_single: two-stage parameters (tspws_hip_jackknife takes those)");
	if (mtr && ld < pl->N) return fail(TSPWS_E_ARG, "jackknife_single: row stride below the trace length");
	if (!C) return 0;
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	const size_t N = pl->N, nc = pl->ncoef;
	int rc;
	void *v;

	// classes (host): class of every trace, kept[C][ncls], the traces of each class in trace order (idx, cptr)
	std::vector<unsigned> cls(mtr);
	std::vector<char> kept((size_t)C * std::max<size_t>(mtr, 1));
	unsigned ncls = 0;
	if ((rc = tspws_selection_classes(h_sel, C, mtr, cls.data(), kept.data(), &ncls))) return rc;
	if (ncls > 65535) return fail(TSPWS_E_ARG, "jackknife_single: more than 65535 distinct selection columns");
	std::vector<unsigned> Kc(C, 0);
	for (unsigned c = 0; c < C; c++) {
		const char *row = h_sel + (size_t)c * mtr;
		unsigned n = 0;
		for (size_t i = 0; i < mtr; i++) n += row[i] == 1;
		Kc[c] = n;
		h_mtr_out[c] = n;
	}
	std::vector<unsigned> cptr(ncls + 1, 0), idx(mtr);
	for (size_t i = 0; i < mtr; i++) cptr[cls[i] + 1]++;
	for (unsigned k = 0; k < ncls; k++) cptr[k + 1] += cptr[k];
	{
		std::vector<unsigned> fill(cptr.begin(), cptr.end() - 1);
		for (size_t i = 0; i < mtr; i++) idx[fill[cls[i]]++] = (unsigned)i;
	}
	// forward batches: as many traces as the parts budget holds (TSPWS_PART_MB); per batch and class the range of its traces in idx
	const size_t budget = tspws_part_budget_bytes();
	const size_t FB = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(mtr, 1), budget / (pl->npart * sizeof(double2))));
	const size_t nbat = (mtr + FB - 1) / FB;
	std::vector<unsigned> rg(nbat * ncls * 2);
	for (unsigned k = 0; k < ncls; k++) {
		unsigned q = cptr[k];
		for (size_t b = 0; b < nbat; b++) {
			const size_t t1 = std::min(mtr, (b + 1) * FB);
			rg[(b * ncls + k) * 2] = q;
			while (q < cptr[k + 1] && idx[q] < t1) q++;
			rg[(b * ncls + k) * 2 + 1] = q;
		}
	}
	// one table block: idx | cptr | ranges (8-byte aligned: uint2) | Kc | kept
	const size_t o_cp = mtr * 4, o_rg = (o_cp + (ncls + 1) * 4 + 7) & ~(size_t)7, o_kc = o_rg + rg.size() * 4, o_kp = o_kc + (size_t)C * 4;
	std::vector<char> blob(o_kp + (size_t)C * ncls + 1);
	if (mtr) memcpy(blob.data(), idx.data(), mtr * 4);
	memcpy(blob.data() + o_cp, cptr.data(), (ncls + 1) * 4);
	if (!rg.empty()) memcpy(blob.data() + o_rg, rg.data(), rg.size() * 4);
	memcpy(blob.data() + o_kc, Kc.data(), (size_t)C * 4);
	if (ncls) memcpy(blob.data() + o_kp, kept.data(), (size_t)C * ncls);
	if ((rc = scratch(pl, SCR_J1TAB, blob.size(), &v))) return rc;
	char *tb = (char *)v;
	HIP_TRY(hipMemcpyAsync(tb, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
	const unsigned *d_idx = (const unsigned *)tb, *d_cptr = (const unsigned *)(tb + o_cp), *d_Kc = (const unsigned *)(tb + o_kc);
	const uint2 *d_rg = (const uint2 *)(tb + o_rg);
	const char *d_kept = tb + o_kp;

	// class pass: plane pairs and time sums of every class
	double2 *planes = nullptr;
	double *T = nullptr;
	if (ncls) {
		if ((rc = scratch(pl, SCR_J1PL, (size_t)ncls * 2 * nc * sizeof(double2), &v))) return rc;
		planes = (double2 *)v;
		if ((rc = scratch(pl, SCR_J1T, (size_t)ncls * N * sizeof(double), &v))) return rc;
		T = (double *)v;
		HIP_TRY(hipMemsetAsync(planes, 0, (size_t)ncls * 2 * nc * sizeof(double2), st));
		if ((rc = scratch(pl, SCR_PART, FB * pl->npart * sizeof(double2), &v))) return rc;
		double2 *part = (double2 *)v;
		for (size_t b = 0; b < nbat; b++) {
			const size_t t0 = b * FB, nf = std::min(FB, mtr - t0);
			if ((rc = tspws_forward_parts<float>(pl, d_x + t0 * ld, nf, ld, part, st, nullptr, ScaleRange()))) return rc;
			hipLaunchKernelGGL(k_j1_accumulate, dim3(pl->acc_blocks, ncls), dim3(256), 0, st, (const double2 *)part, pl->npart, (const ScaleDesc *)pl->d_sc, pl->S,
			                   nc, d_rg + b * ncls, d_idx, t0, planes);
		}
		hipLaunchKernelGGL(k_j1_time, dim3((unsigned)((N + 255) / 256), ncls), dim3(256), 0, st, d_x, ld, N, d_idx, d_cptr, T);
	}

	// replicas in batches of RB (weighted sets + reconstructions within the parts budget; even, so that the inverse pairs the same
	// replicas whatever the batching)
	const size_t per_rep = nc * sizeof(double2) + N * sizeof(double);
	unsigned RB = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(C, 65534), budget / per_rep)); // (grid.y of k_j1_linear)
	if (RB > 1) RB &= ~1u;
	if ((rc = scratch(pl, SCR_JKOUT, (size_t)RB * per_rep, &v))) return rc;
	double *OUT = (double *)v, *xr = OUT + (size_t)RB * 2 * nc;
	const bool lds = ncls <= J1_LDS_MAX;
	for (unsigned c0 = 0; c0 < C && ncls; c0 += RB) {
		const unsigned nr = std::min(RB, C - c0);
		const dim3 grid((unsigned)((nc + J1_NT - 1) / J1_NT), (nr + J1_RPB - 1) / J1_RPB);
		if (lds)
			hipLaunchKernelGGL(k_j1_finish<true>, grid, dim3(J1_NT), (size_t)ncls * 2 * J1_NT * sizeof(double2), st, (const double2 *)planes, ncls, nc, d_kept,
			                   d_Kc, c0, nr, p->wu, p->unbiased, (double2 *)OUT);
		else
			hipLaunchKernelGGL(k_j1_finish<false>, grid, dim3(J1_NT), 0, st, (const double2 *)planes, ncls, nc, d_kept, d_Kc, c0, nr, p->wu, p->unbiased,
			                   (double2 *)OUT);
		if ((rc = tspws_hip_inverse(pl, OUT, nr, xr, s))) return rc;
		tspws_epilogue_rows(d_ts_out + (size_t)c0 * N, xr, N, nr, st);
		hipLaunchKernelGGL(k_j1_linear, dim3((unsigned)((N + 255) / 256), nr), dim3(256), 0, st, (const double *)T, N, ncls, d_kept, d_Kc, c0, d_ls_out);
	}
	// replicas without traces: zero rows (the reference has no answer here)
	for (unsigned c = 0; c < C; c++)
		if (!Kc[c]) {
			HIP_TRY(hipMemsetAsync(d_ls_out + (size_t)c * N, 0, N * sizeof(float), st));
			HIP_TRY(hipMemsetAsync(d_ts_out + (size_t)c * N, 0, N * sizeof(float), st));
		}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st)); // outputs complete; the host tables above go out of scope
	return 0;
}
