// jk_batch.hip -- the single-stage jackknife of many ensembles in one call (tspws_hip_jackknife_batch).
//
// tspws_hip_stack_batch stacks B ensembles in one many-trace pass and gives no uncertainty; tspws_hip_jackknife_single gives the delete-d
// replicas of ONE ensemble.  This unit joins them: to the shared many-trace pass of batch.hip a (ensemble, class) is one more "ensemble"
// (class = the traces of an ensemble whose selection columns are identical, jk_single.hip), and every replica of every ensemble is a sum of
// that ensemble's class planes.
//   host          classes of every ensemble from its column range of the selection (first-appearance order), flattened into one list;
//                 every class starts a fresh 64-trace block, its traces in trace order in the first lanes (src = -1: idle lane)
//   shared pass   tspws_tl_pass_setup / _transform on the gathered batches, engine by the TOTAL trace count; k_jb_accumulate adds each
//                 class's block planes / per-trace partials into the class's own [ST | PS] pair (the arithmetic of k_accumulate_parts for
//                 a many-trace table without weights; ONE launch per batch of the pass: grid.y = segment, a descriptor per segment, so
//                 classes of 28 / 30 / 31 traces do not cost a launch each); a class that straddles two batches keeps accumulating
//   time sums     k_j1_time over the flat class list: the FP64 sums behind the replicas' linear stacks
//   finish        k_jb_finish per (coefficient tile, row group, ensemble): ST_c / PS_c = sums of the kept classes' planes in class order,
//                 weight with K = M = K_c; the main rows, when wanted, are the all-classes sum with K = M = M_b as an (OUT, ST) pair in
//                 front of the replicas; one batched tspws_hip_inverse per batch of rows; k_jb_epilogue (replicas: the float cast; main
//                 rows: ls by a FLOAT division by M_b); k_jb_linear for the replicas' linear stacks
// Rounds keep every scratch block that grows with the ensembles -- class planes, time sums, weighted sets, reconstructions, the inverse's
// octave buffer, tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble (one ensemble alone may exceed it
// with its class planes), and the rows of a round go through the finish in even batches.  A batch whose total trace count does not take
// the many-trace path is one tspws_hip_stack + tspws_hip_jackknife_single per ensemble.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

#define is_two_stage tspws_is_two_stage

namespace {

struct JbSeg { unsigned blk, nblk, ntr, cls, head; };           // blocks [blk, blk + nblk) of a pass batch hold ntr traces of class cls (of the round)

} // namespace

// Class planes of one batch of the many-trace pass: segment blockIdx.y adds its blocks' plane pairs (fused scales: slice order) and its
// traces' partials (the other scales: a wave per coefficient, the lanes take every 64th trace, then a wave reduction) into the plane pair
// of its class -- k_accumulate_parts' `fused == 2` and `wide && many` branches with a descriptor per segment instead of one geometry per launch.
__global__ void __launch_bounds__(256) k_jb_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                       size_t ncoef, const double2 *__restrict__ fz, const JbSeg *__restrict__ seg,
                                                       double2 *__restrict__ planes)
{
	const JbSeg s = seg[blockIdx.y];
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, true);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	double2 *ST = planes + (size_t)s.cls * 2 * ncoef, *PS = ST + ncoef;
	if (sc[lo].fuse_ok) {
		const unsigned k = (blockIdx.x - sc[lo].acc2_off) * 256u + threadIdx.x;
		if (k >= Ns) return;
		const size_t i = sc[lo].coef_off + k;
		double2 st = make_double2(0, 0), ps = make_double2(0, 0);
		if (!s.head) { st = ST[i]; ps = PS[i]; }
		const double2 *f = fz + (size_t)s.blk * 2 * ncoef + i;
		for (unsigned j = 0; j < s.nblk; j++) {
			const double2 a = f[(size_t)j * 2 * ncoef], b = f[(size_t)j * 2 * ncoef + ncoef];
			st.x += a.x; st.y += a.y; ps.x += b.x; ps.y += b.y;
		}
		ST[i] = st; PS[i] = ps;
		return;
	}
	const unsigned k = (blockIdx.x - sc[lo].acc2_off) * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const double2 *p0 = part + (size_t)s.blk * 64 * npart + sc[lo].part_off + k;
	double2 st = make_double2(0, 0), ps = make_double2(0, 0);
	for (unsigned b = lane; b < s.ntr; b += 64) {
		const double2 *p = p0 + (size_t)b * npart;
		double2 v = make_double2(0.0, 0.0);
		for (unsigned sp = 0; sp < nsplit; sp++) { const double2 t = p[(size_t)sp * Ns]; v.x += t.x; v.y += t.y; }
		st.x += v.x; st.y += v.y;
		add_unit_phasor(ps, v);
	}
	st.x = wave_sum(st.x); st.y = wave_sum(st.y); ps.x = wave_sum(ps.x); ps.y = wave_sum(ps.y);
	if (lane == 0) {
		if (!s.head) { const double2 a = ST[i], b = PS[i]; st.x += a.x; st.y += a.y; ps.x += b.x; ps.y += b.y; }
		ST[i] = st; PS[i] = ps;
	}
}

// float outputs of the rows of k_jb_finish after the inverse: x[(z nq + y)][n] = reconstruction of row q0 + y of ensemble z.  Main rows:
// tsPWS = (float) ICWT(OUT), ls = (float) ICWT(ST) / (float) M_b (ts_pws1f_lib.c:233-241); replicas: tsPWS_out = (float) x (zero rows for K_c = 0)
__global__ void __launch_bounds__(256) k_jb_epilogue(const double *__restrict__ x, size_t N, const JbEns *__restrict__ ens, const unsigned *__restrict__ Kc,
                                                     unsigned C, unsigned main, unsigned q0, unsigned nq, float *__restrict__ ls, float *__restrict__ ts,
                                                     float *__restrict__ ts_out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const JbEns e = ens[blockIdx.z];
	const unsigned q = q0 + blockIdx.y;
	const double v = x[((size_t)blockIdx.z * nq + blockIdx.y) * N + n];
	if (q < 2 * main) {
		if (q == 0) ts[(size_t)e.row * N + n] = (float)v;
		else ls[(size_t)e.row * N + n] = (float)v / (float)e.M;
	} else {
		const unsigned c = q - 2 * main;
		ts_out[((size_t)e.row * C + c) * N + n] = Kc[e.kc_off + c] ? (float)v : 0.f;
	}
}

namespace {

struct Ens { unsigned b; size_t f, m, cls0, ncls, kept_off; }; // ensemble with traces: index, first trace, traces, classes [cls0, cls0 + ncls) of the call, kept[C][ncls]

struct Layout {
	std::vector<Ens> ens;
	std::vector<unsigned> idx;    // global trace indices, class by class, trace order inside a class
	std::vector<size_t> cptr;     // class g = idx[cptr[g], cptr[g + 1])
	std::vector<size_t> blk0;     // blocks of class g = [blk0[g], blk0[g + 1])
	std::vector<char> kept;       // per ensemble [C][ncls]
};

// the tables of a round in one block: gather slots | ensembles | segments of every batch of the pass | idx | cptr | K_c | kept
struct JbTab { size_t src, ens, seg, idx, cp, kc, kept, bytes; };
JbTab jb_tab(size_t nslots, size_t ne, size_t nseg, size_t ntr, size_t ncl, size_t nkc, size_t nkept)
{
	TableLayout lay;
	const size_t src = lay.add<long long>(nslots), ens = lay.add<JbEns>(ne), seg = lay.add<JbSeg>(nseg), idx = lay.add<unsigned>(ntr),
	             cp = lay.add<unsigned>(ncl + 1), kc = lay.add<unsigned>(nkc), kept = lay.add<char>(nkept);
	return {src, ens, seg, idx, cp, kc, kept, lay.bytes};
}

int shared_pass(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const Layout &L, size_t total, unsigned C, bool main, float *d_ls,
                float *d_ts, float *d_ls_out, float *d_ts_out, const unsigned *h_Kc, BatchCall &call)
{
	const size_t N = pl->N, nc = pl->ncoef, n = L.ens.size(), G = L.cptr.size() - 1;
	hipStream_t st = call.stream();
	const size_t budget = tspws_part_budget_bytes();
	const unsigned RPE = C + (main ? 2u : 0u); // rows of an ensemble
	int rc;
	void *v;
	TlPass P;
	if ((rc = tspws_tl_pass_setup<float>(pl, total, L.blk0[G] * 64, P))) return rc;
	const TlTable &T = *P.T;
	const size_t bpb = P.batch / 64; // blocks per batch of the pass
	if ((rc = scratch(pl, SCR_BXG, P.batch * N * sizeof(float), &v))) return rc;
	float *xg = (float *)v;

	// rounds of whole ensembles: class planes, time sums, two rows per ensemble of sets / reconstructions / octave buffer and the tables within
	// the budget; at most 65535 classes and ensembles (grid.y / grid.z)
	const size_t per_row = tspws_inverse_row_bytes(pl);
	auto cls_end = [&](size_t j) { return L.ens[j].cls0 + L.ens[j].ncls; };
	auto tab_bound = [&](size_t j0, size_t j1) { // (a class has at most one segment per batch it touches)
		const size_t g0 = L.ens[j0].cls0, ncl = cls_end(j1 - 1) - g0, nblk = L.blk0[g0 + ncl] - L.blk0[g0];
		return jb_tab(nblk * 64, j1 - j0, ncl + nblk / bpb + 2, L.cptr[g0 + ncl] - L.cptr[g0], ncl, (j1 - j0) * C, (size_t)C * ncl).bytes;
	};
	const std::vector<Round> rounds = whole_ensemble_rounds(n, [&](size_t j0, size_t j1) {
		const size_t ncl = cls_end(j1 - 1) - L.ens[j0].cls0, ne = j1 - j0;
		return !(ncl > 65535 || ne > 65535 || ncl * 2 * nc * sizeof(double2) > budget || ncl * N * sizeof(double) > budget || ne * 2 * per_row > budget ||
		         tab_bound(j0, j1) > budget);
	});
	// rows per ensemble and finish batch
	auto rows_per_batch = [&](size_t ne) { return (unsigned)even_rows_per_batch(budget, ne * per_row, RPE); };
	size_t max_cls = 0, max_rows = 0, max_tab = 0;
	for (const Round &r : rounds) {
		max_cls = std::max(max_cls, cls_end(r.j1 - 1) - L.ens[r.j0].cls0);
		max_rows = std::max(max_rows, (r.j1 - r.j0) * rows_per_batch(r.j1 - r.j0));
		max_tab = std::max(max_tab, tab_bound(r.j0, r.j1));
	}
	if ((rc = scratch(pl, SCR_JBPL, max_cls * 2 * nc * sizeof(double2), &v))) return rc;
	double2 *planes = (double2 *)v;
	if ((rc = scratch(pl, SCR_JBT, max_cls * N * sizeof(double), &v))) return rc;
	double *Tsum = (double *)v;
	if ((rc = scratch(pl, SCR_ROWY, max_rows * nc * sizeof(double2), &v))) return rc;
	double2 *OUT = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWX, max_rows * N * sizeof(double), &v))) return rc;
	double *xr = (double *)v;

	for (const Round &r : rounds) {
		const size_t ne = r.j1 - r.j0, g0 = L.ens[r.j0].cls0, g1 = cls_end(r.j1 - 1), ncl = g1 - g0;
		const size_t b0 = L.blk0[g0], b1 = L.blk0[g1], q0r = L.cptr[g0], ntr = L.cptr[g1] - q0r;
		pl->jk_batch_stats.rounds++;
		// the round's tables
		std::vector<JbSeg> segs;
		std::vector<size_t> seg0; // segments of batch k: [seg0[k], seg0[k + 1])
		for (size_t c0 = b0; c0 < b1; c0 += bpb) {
			const size_t c1 = std::min(b1, c0 + bpb);
			seg0.push_back(segs.size());
			size_t g = std::upper_bound(L.blk0.begin(), L.blk0.end(), c0) - L.blk0.begin() - 1;
			for (; g < g1 && L.blk0[g] < c1; g++) {
				const size_t m = L.cptr[g + 1] - L.cptr[g], s0 = std::max(L.blk0[g], c0), s1 = std::min(L.blk0[g + 1], c1);
				JbSeg s;
				s.blk = (unsigned)(s0 - c0); s.nblk = (unsigned)(s1 - s0);
				s.ntr = (unsigned)(std::min(m, (s1 - L.blk0[g]) * 64) - (s0 - L.blk0[g]) * 64);
				s.cls = (unsigned)(g - g0); s.head = s0 == L.blk0[g] ? 1u : 0u;
				segs.push_back(s);
			}
		}
		seg0.push_back(segs.size());
		const JbTab o = jb_tab((b1 - b0) * 64, ne, segs.size(), ntr, ncl, ne * C, (size_t)C * ncl);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, "jackknife_batch: table bound"); // (cannot happen: tab_bound is an upper bound)
		char *blob = call.block(o.bytes), *tab;
		long long *src = (long long *)(blob + o.src);
		JbEns *he = (JbEns *)(blob + o.ens);
		unsigned *hidx = (unsigned *)(blob + o.idx), *hcp = (unsigned *)(blob + o.cp), *hkc = (unsigned *)(blob + o.kc);
		if (!segs.empty()) memcpy(blob + o.seg, segs.data(), segs.size() * sizeof(JbSeg));
		for (size_t g = g0; g < g1; g++) {
			const size_t m = L.cptr[g + 1] - L.cptr[g];
			for (size_t i = 0; i < (L.blk0[g + 1] - L.blk0[g]) * 64; i++) src[(L.blk0[g] - b0) * 64 + i] = i < m ? (long long)L.idx[L.cptr[g] + i] : -1;
			hcp[g - g0] = (unsigned)(L.cptr[g] - q0r);
		}
		hcp[ncl] = (unsigned)ntr;
		memcpy(hidx, L.idx.data() + q0r, ntr * 4);
		size_t kp = 0;
		unsigned max_ncls = 0;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = L.ens[j];
			JbEns d;
			d.cls0 = (unsigned)(e.cls0 - g0); d.ncls = (unsigned)e.ncls; d.kept_off = (unsigned)kp; d.kc_off = (unsigned)((j - r.j0) * C);
			d.M = (unsigned)e.m; d.row = e.b;
			he[j - r.j0] = d;
			memcpy(hkc + (j - r.j0) * (size_t)C, h_Kc + (size_t)e.b * C, (size_t)C * 4);
			memcpy(blob + o.kept + kp, L.kept.data() + e.kept_off, (size_t)C * e.ncls);
			kp += (size_t)C * e.ncls;
			max_ncls = std::max(max_ncls, d.ncls);
		}
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const long long *d_src = (const long long *)(tab + o.src);
		const JbEns *d_ens = (const JbEns *)(tab + o.ens);
		const JbSeg *d_seg = (const JbSeg *)(tab + o.seg);
		const unsigned *d_idx = (const unsigned *)(tab + o.idx), *d_cp = (const unsigned *)(tab + o.cp), *d_kc = (const unsigned *)(tab + o.kc);
		const char *d_kept = tab + o.kept;

		// class pass: the round's blocks in batches of the pass (whole blocks: a class may straddle two batches)
		size_t kb = 0;
		for (size_t c0 = b0; c0 < b1; c0 += bpb, kb++) {
			const size_t c1 = std::min(b1, c0 + bpb);
			const unsigned nb = (unsigned)((c1 - c0) * 64), nseg = (unsigned)(seg0[kb + 1] - seg0[kb]);
			pl->jk_batch_stats.pass_batches++;
			hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, d_x, ld, d_src + (c0 - b0) * 64, (unsigned)N, xg);
			if ((rc = tspws_tl_pass_transform<float>(pl, P, xg, N, nb, st))) return rc;
			hipLaunchKernelGGL(k_jb_accumulate, dim3(T.acc2_blocks, nseg), dim3(256), 0, st, (const double2 *)P.part, T.npart, (const ScaleDesc *)T.d_sc, pl->S, nc,
			                   (const double2 *)P.planes, d_seg + seg0[kb], planes);
		}
		hipLaunchKernelGGL(k_j1_time, dim3((unsigned)((N + 255) / 256), (unsigned)ncl), dim3(256), 0, st, d_x, ld, N, d_idx, d_cp, Tsum);

		// finish: the rows of every ensemble in even batches
		const unsigned RB = rows_per_batch(ne), mn = main ? 1u : 0u;
		const bool lds = max_ncls <= JB_LDS_MAX;
		for (unsigned q0 = 0; q0 < RPE; q0 += RB) {
			const unsigned nq = std::min(RB, RPE - q0);
			const dim3 grid((unsigned)((nc + JB_NT - 1) / JB_NT), (nq + JB_RPB - 1) / JB_RPB, (unsigned)ne);
			if (lds)
				hipLaunchKernelGGL(k_jb_finish<true>, grid, dim3(JB_NT), (size_t)max_ncls * 2 * JB_NT * sizeof(double2), st, (const double2 *)planes, nc, d_ens, d_kept,
				                   d_kc, mn, q0, nq, p->wu, p->unbiased, OUT);
			else
				hipLaunchKernelGGL(k_jb_finish<false>, grid, dim3(JB_NT), 0, st, (const double2 *)planes, nc, d_ens, d_kept, d_kc, mn, q0, nq, p->wu, p->unbiased, OUT);
			if ((rc = tspws_hip_inverse(pl, (const double *)OUT, ne * nq, xr, (void *)st))) return rc;
			hipLaunchKernelGGL(k_jb_epilogue, dim3((unsigned)((N + 255) / 256), nq, (unsigned)ne), dim3(256), 0, st, (const double *)xr, N, d_ens, d_kc, C, mn, q0, nq,
			                   d_ls, d_ts, d_ts_out);
		}
		for (unsigned c0 = 0; c0 < C; c0 += 65535)
			hipLaunchKernelGGL(k_jb_linear, dim3((unsigned)((N + 255) / 256), std::min(65535u, C - c0), (unsigned)ne), dim3(256), 0, st, (const double *)Tsum, N, d_ens,
			                   d_kept, d_kc, C, c0, d_ls_out);
	}
	return 0;
}

} // namespace

extern "C" int tspws_hip_jackknife_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                                         const char *h_sel, unsigned C, float *d_ls, float *d_ts, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out,
                                         void *s)
{
	// (the checks that need no plan come first: a host without a device can see every one of them refuse)
	if (!p || !h_first) return fail(TSPWS_E_ARG, "jackknife_batch: NULL");
	if (!B || !C) return pl ? 0 : fail(TSPWS_E_ARG, "jackknife_batch: NULL");
	if (!h_sel || !d_ls_out || !d_ts_out || !h_mtr_out) return fail(TSPWS_E_ARG, "jackknife_batch: NULL");
	if (!d_ls != !d_ts) return fail(TSPWS_E_ARG, "jackknife_batch: exactly one of the main outputs is NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "jackknife_batch: decreasing ensemble offsets");
	for (unsigned b = 0; b < B; b++)
		if (is_two_stage(p, h_first[b + 1] - h_first[b]))
			return fail(TSPWS_E_ARG, "jackknife_batch: two-stage parameters for an ensemble (tspws_hip_jackknife takes those)");
	if (h_first[B] > 0xffffffffull) return fail(TSPWS_E_ARG, "jackknife_batch: trace indices beyond 32 bits");
	const size_t Tn = h_first[B] - h_first[0];
	const bool main = d_ls != nullptr;

	// classes of every ensemble, flattened: class g of the call = idx[cptr[g], cptr[g + 1]), blocks [blk0[g], blk0[g + 1])
	Layout L;
	L.cptr.push_back(0);
	L.blk0.push_back(0);
	L.idx.reserve(Tn);
	std::vector<unsigned> cls;
	std::vector<size_t> firsts;
	unsigned nempty = 0;
	for (unsigned b = 0; b < B; b++) {
		const size_t f = h_first[b], m = h_first[b + 1] - f, col0 = f - h_first[0];
		if (!m) { nempty++; continue; }
		cls.resize(m);
		selection_classes_strided(h_sel, C, Tn, col0, m, cls.data(), firsts);
		const size_t ncls = firsts.size();
		if (ncls > 65535) return fail(TSPWS_E_ARG, "jackknife_batch: more than 65535 distinct selection columns in one ensemble");
		Ens e;
		e.b = b; e.f = f; e.m = m; e.cls0 = L.cptr.size() - 1; e.ncls = ncls; e.kept_off = L.kept.size();
		L.kept.resize(e.kept_off + (size_t)C * ncls);
		for (unsigned c = 0; c < C; c++)
			for (size_t k = 0; k < ncls; k++) L.kept[e.kept_off + (size_t)c * ncls + k] = h_sel[(size_t)c * Tn + col0 + firsts[k]] == 1 ? 1 : 0;
		std::vector<size_t> cnt(ncls + 1, 0);
		for (size_t i = 0; i < m; i++) cnt[cls[i] + 1]++;
		for (size_t k = 0; k < ncls; k++) cnt[k + 1] += cnt[k];
		const size_t base = L.idx.size();
		L.idx.resize(base + m);
		for (size_t k = 0; k < ncls; k++) {
			L.cptr.push_back(base + cnt[k + 1]);
			L.blk0.push_back(L.blk0.back() + (cnt[k + 1] - cnt[k] + 63) / 64);
		}
		for (size_t i = 0; i < m; i++) L.idx[base + cnt[cls[i]]++] = (unsigned)(f + i);
		L.ens.push_back(e);
	}
	if (!pl) return fail(TSPWS_E_ARG, "jackknife_batch: NULL");
	const size_t N = pl->N;
	if (Tn && !d_x) return fail(TSPWS_E_ARG, "jackknife_batch: NULL traces");
	if (Tn && ld < N) return fail(TSPWS_E_ARG, "jackknife_batch: row stride below the trace length");
	// replica sizes
	for (unsigned b = 0; b < B; b++) {
		const size_t col0 = h_first[b] - h_first[0], m = h_first[b + 1] - h_first[b];
		for (unsigned c = 0; c < C; c++) h_mtr_out[(size_t)b * C + c] = kept_count(h_sel + (size_t)c * Tn + col0, m);
	}
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	int rc;
	pl->jk_batch_stats = tspws_hip_jk_batch_stats();
	pl->jk_batch_stats.empty = nempty;
	pl->jk_batch_stats.classes = (unsigned)(L.cptr.size() - 1);
	BatchCall call(st);
	if (!L.ens.empty() && tspws_many_trace_path(pl, Tn)) {
		pl->jk_batch_stats.shared = (unsigned)L.ens.size();
		if ((rc = shared_pass(pl, p, d_x, ld, L, Tn, C, main, d_ls, d_ts, d_ls_out, d_ts_out, h_mtr_out, call))) return rc;
	} else {
		pl->jk_batch_stats.looped = (unsigned)L.ens.size();
		for (const Ens &e : L.ens) {
			const char *sel = ensemble_selection(call, h_sel, C, Tn, e.f - h_first[0], e.m);
			if (main && (rc = tspws_hip_stack(pl, p, d_x + e.f * ld, ld, e.m, d_ls + (size_t)e.b * N, d_ts + (size_t)e.b * N, s))) return rc;
			if ((rc = tspws_hip_jackknife_single(pl, p, d_x + e.f * ld, ld, e.m, sel, C, d_ls_out + (size_t)e.b * C * N, d_ts_out + (size_t)e.b * C * N,
			                                     h_mtr_out + (size_t)e.b * C, s)))
				return rc;
		}
	}
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls_out, (size_t)C * N}, {d_ts_out, (size_t)C * N}, {d_ls, N}, {d_ts, N}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_jackknife_batch_stats(const tspws_hip_plan *pl, tspws_hip_jk_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "jackknife_batch_stats: NULL");
	*stats = pl->jk_batch_stats;
	return 0;
}
