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
//                replica's own K_c (k_jb_finish, batch_kernels.h, for one ensemble without main rows: a coefficient's class values are
//                staged once in LDS for RPB replicas), the batched inverse, the float epilogue; ls_c from the class time sums (k_jb_linear).
// FP64 summation order: by class, then over the kept classes in class order (not trace order); the float outputs agree with a
// trace-order restatement to the last bits.  A replica without traces (K_c = 0) gets zero rows and count 0.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

#define is_two_stage tspws_is_two_stage

// ------------------------------------------------------------------------------------------
// host: classes of a selection
// ------------------------------------------------------------------------------------------
extern "C" int tspws_selection_classes(const char *sel, unsigned C, size_t mtr, unsigned *class_of_trace, char *kept, unsigned *ncls)
{
	if (!sel || !class_of_trace || !ncls) return fail(TSPWS_E_ARG, "selection_classes: NULL");
	std::vector<size_t> first; // first trace of every class
	selection_classes_strided(sel, C, mtr, 0, mtr, class_of_trace, first);
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
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, false);
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
	// forward batches: as many traces as the parts budget holds (TSPWS_PART_MB); per batch and class the range of its traces in idx
	const size_t budget = tspws_part_budget_bytes();
	const size_t FB = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(mtr, 1), budget / (pl->npart * sizeof(double2))));
	const size_t nbat = (mtr + FB - 1) / FB;
	// one table block: idx | cptr | ranges | Kc | kept | the one ensemble descriptor of the batched finish kernels
	TableLayout lay;
	const size_t o_idx = lay.add<unsigned>(mtr), o_cp = lay.add<unsigned>(ncls + 1), o_rg = lay.add<uint2>(nbat * ncls), o_kc = lay.add<unsigned>(C),
	             o_kp = lay.add<char>((size_t)C * ncls), o_ens = lay.add<JbEns>(1);
	BatchCall call(st);
	char *blob = call.block(lay.bytes), *tb;
	unsigned *idx = (unsigned *)(blob + o_idx), *cptr = (unsigned *)(blob + o_cp), *rg = (unsigned *)(blob + o_rg), *Kc = (unsigned *)(blob + o_kc);
	for (unsigned c = 0; c < C; c++) Kc[c] = h_mtr_out[c] = kept_count(h_sel + (size_t)c * mtr, mtr);
	for (size_t i = 0; i < mtr; i++) cptr[cls[i] + 1]++;
	for (unsigned k = 0; k < ncls; k++) cptr[k + 1] += cptr[k];
	{
		std::vector<unsigned> fill(cptr, cptr + ncls);
		for (size_t i = 0; i < mtr; i++) idx[fill[cls[i]]++] = (unsigned)i;
	}
	for (unsigned k = 0; k < ncls; k++) {
		unsigned q = cptr[k];
		for (size_t b = 0; b < nbat; b++) {
			const size_t t1 = std::min(mtr, (b + 1) * FB);
			rg[(b * ncls + k) * 2] = q;
			while (q < cptr[k + 1] && idx[q] < t1) q++;
			rg[(b * ncls + k) * 2 + 1] = q;
		}
	}
	if (ncls) memcpy(blob + o_kp, kept.data(), (size_t)C * ncls);
	*(JbEns *)(blob + o_ens) = JbEns{0, ncls, 0, 0, 0, 0}; // every class, kept / K_c / output rows from the start; M only weighs main rows
	if ((rc = call.upload(pl, SCR_J1TAB, blob, lay.bytes, &tb))) return rc;
	const unsigned *d_idx = (const unsigned *)(tb + o_idx), *d_cptr = (const unsigned *)(tb + o_cp), *d_Kc = (const unsigned *)(tb + o_kc);
	const uint2 *d_rg = (const uint2 *)(tb + o_rg);
	const char *d_kept = tb + o_kp;
	const JbEns *d_ens = (const JbEns *)(tb + o_ens);

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
	unsigned RB = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(C, 65534), budget / per_rep)); // (grid.y of k_jb_linear)
	if (RB > 1) RB &= ~1u;
	if ((rc = scratch(pl, SCR_JKOUT, (size_t)RB * per_rep, &v))) return rc;
	double *OUT = (double *)v, *xr = OUT + (size_t)RB * 2 * nc;
	const bool lds = ncls <= JB_LDS_MAX;
	for (unsigned c0 = 0; c0 < C && ncls; c0 += RB) {
		const unsigned nr = std::min(RB, C - c0);
		const dim3 grid((unsigned)((nc + JB_NT - 1) / JB_NT), (nr + JB_RPB - 1) / JB_RPB);
		if (lds)
			hipLaunchKernelGGL(k_jb_finish<true>, grid, dim3(JB_NT), (size_t)ncls * 2 * JB_NT * sizeof(double2), st, (const double2 *)planes, nc, d_ens, d_kept,
			                   d_Kc, 0u, c0, nr, p->wu, p->unbiased, (double2 *)OUT);
		else
			hipLaunchKernelGGL(k_jb_finish<false>, grid, dim3(JB_NT), 0, st, (const double2 *)planes, nc, d_ens, d_kept, d_Kc, 0u, c0, nr, p->wu, p->unbiased,
			                   (double2 *)OUT);
		if ((rc = tspws_hip_inverse(pl, OUT, nr, xr, s))) return rc;
		tspws_epilogue_rows(d_ts_out + (size_t)c0 * N, xr, N, nr, st);
		hipLaunchKernelGGL(k_jb_linear, dim3((unsigned)((N + 255) / 256), nr), dim3(256), 0, st, (const double *)T, N, d_ens, d_kept, d_Kc, C, c0, d_ls_out);
	}
	// replicas without traces: zero rows (the reference has no answer here)
	for (unsigned c = 0; c < C; c++)
		if (!Kc[c]) {
			HIP_TRY(hipMemsetAsync(d_ls_out + (size_t)c * N, 0, N * sizeof(float), st));
			HIP_TRY(hipMemsetAsync(d_ts_out + (size_t)c * N, 0, N * sizeof(float), st));
		}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}
