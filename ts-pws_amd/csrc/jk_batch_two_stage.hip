// jk_batch_two_stage.hip -- the two-stage jackknife of many ensembles in one call (tspws_hip_jackknife_batch_two_stage).
// Reference citations are relative to the reference project's src/ directory.
//
// tspws_hip_stack_batch stacks B small ensembles in one launch sequence, tspws_hip_jackknife_batch gives their single-stage replicas; the
// jackknife the reference implements (TwoStage_jackknife_float, ts_pws1f_lib.c:719-831) was left to a loop of tspws_hip_stack_jackknife:
// per ensemble a new selection for the masked-replica tables (resample.hip keeps ONE per host thread), an upload, a wait, and a handful of
// 5-40 us launches on ~130 rows.  This unit does the whole batch at once:
//   host      ONE pass over the selection: per ensemble and column (replica; the plain stack as column C) the piecewise-constant group
//             signature -- the rule and the builders the masked replicas of a single ensemble use too (column_runs.h); the columns in tiles
//             of <= 16, the traces of an (ensemble, tile) cut into runs of one signature
//   walk      k_jb2_rows_walk: a workgroup owns one (ensemble, tile, 1024 samples), walks the ensemble's traces once in trace order with a
//             running FP64 sum per column in registers (16 columns x 4 samples per lane); at the end of a run the run's sum goes to the
//             columns it belongs to (wave-uniform bit tests), and a column whose group ends there stores its sum as that group's row and
//             starts over.  Direct stores; no atomics: every row has one writer.  Rows nobody reaches (empty groups, K_c = 0) are zero: the
//             round's row block is cleared first when it has one.
//   rows      of a round, replica-major: [(ensemble, replica)][Kmax][N], then [(ensemble) plain stack][Kmax][N] -- a slice of Kmax rows per column
//   finish    one tspws_forward_parts<double> over all rows of the round (fused slices of Kmax rows where the plan has a fused kernel), one
//             accumulation, the weights with K = Kmax and each column's own trace count, k_jb2_linear for the replicas' time-domain linear
//             stacks (:799-811), the plain stacks' ST behind their OUT, one batched tspws_hip_inverse, k_jb2_epilogue (replicas: float cast;
//             plain stack: ls by a FLOAT division by M_b)
// Rounds keep every block that grows with the ensembles -- rows, partials, plane pairs, weighted sets, reconstructions, the inverse's octave
// buffer, tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble, one ensemble alone may exceed it.  A batch with
// ONE non-empty ensemble is tspws_hip_stack_jackknife (tspws_hip_jackknife without the main rows) for it.
#include "tspws_internal.h"
#include "batch_host.h"

#define is_two_stage tspws_is_two_stage

namespace {

constexpr unsigned J2_W = 16;          // columns per tile: running sums a lane keeps in registers (16 x 4 doubles)
constexpr int J2_NL = 8;               // independent row loads in flight per lane

struct J2Wg { unsigned run0, run1; };  // the runs of one (ensemble, tile) in the round's run list

} // namespace

typedef float j2_v4f __attribute__((ext_vector_type(4)));

// a run descriptor as wave-uniform values
__device__ __forceinline__ RunDesc j2_run(const RunDesc *__restrict__ runs, unsigned i)
{
	const RunDesc r = runs[i];
	RunDesc u;
	u.t0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(r.t0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)r.t0);
	u.count = (unsigned)__builtin_amdgcn_readfirstlane((int)r.count);
	u.member = (unsigned)__builtin_amdgcn_readfirstlane((int)r.member);
	u.flush = (unsigned)__builtin_amdgcn_readfirstlane((int)r.flush);
	u.frow = (unsigned)__builtin_amdgcn_readfirstlane((int)r.frow);
	u.pad[0] = u.pad[1] = 0;
	return u;
}

// Partial-stack rows of every column of tile blockIdx.y of ensemble blockIdx.z, samples [1024 blockIdx.x, + 1024): the runs [run0, run1) of
// that (ensemble, tile) tile the ensemble's traces in trace order (none is empty).  VEC: 16-byte loads (ld % 4 == 0, 16-byte aligned base); the
// lane that holds the N % 4 tail loads its samples one by one.  The loads do not care where a run ends: batches of J2_NL rows over the whole
// ensemble, a run's end handled inside the batch that holds its last row (the loop of k_rows_walk, stream.hip); the additions keep trace order.
template <bool VEC>
__global__ void __launch_bounds__(256) k_jb2_rows_walk(const float *__restrict__ x, size_t ld, size_t N, const RunDesc *__restrict__ runs,
                                                       const J2Wg *__restrict__ wgs, const unsigned *__restrict__ flush_rows, double *__restrict__ rows)
{
	const size_t col = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
	if (col >= N) return;
	const unsigned rem = (N - col) < 4 ? (unsigned)(N - col) : 4u;
	const J2Wg w = wgs[(size_t)blockIdx.z * gridDim.y + blockIdx.y];
	const unsigned r0 = (unsigned)__builtin_amdgcn_readfirstlane((int)w.run0), r1 = (unsigned)__builtin_amdgcn_readfirstlane((int)w.run1);
	if (r0 >= r1) return;
	const bool pair = !(N & 1) && rem == 4; // 16-byte stores: row * N + col is even
	double P[J2_W][4];
#pragma unroll
	for (int c = 0; c < (int)J2_W; c++)
#pragma unroll
		for (int k = 0; k < 4; k++) P[c][k] = 0;
	double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
	// the end of a run: its sum goes to the columns it belongs to; a column whose group ends there stores its row and starts over
	auto run_end = [&](const RunDesc &rd) {
		unsigned fr = rd.frow;
#pragma unroll
		for (int c = 0; c < (int)J2_W; c++) {
			if ((rd.member >> c) & 1u) { P[c][0] += a0; P[c][1] += a1; P[c][2] += a2; P[c][3] += a3; } // (wave-uniform)
			if ((rd.flush >> c) & 1u) {
				double *dst = rows + (size_t)flush_rows[fr++] * N + col;
				if (pair) { *(double2 *)dst = make_double2(P[c][0], P[c][1]); *(double2 *)(dst + 2) = make_double2(P[c][2], P[c][3]); }
				else {
#pragma unroll
					for (int k = 0; k < 4; k++) if ((unsigned)k < rem) dst[k] = P[c][k];
				}
#pragma unroll
				for (int k = 0; k < 4; k++) P[c][k] = 0;
			}
		}
		a0 = 0; a1 = 0; a2 = 0; a3 = 0;
	};
	const RunDesc first = j2_run(runs, r0), lastd = j2_run(runs, r1 - 1);
	const unsigned long long total = lastd.t0 + lastd.count - first.t0; // traces of the ensemble
	const float *src = x + first.t0 * ld + col;
	auto load = [&](unsigned long long t) -> j2_v4f {
		const float *r = src + (size_t)t * ld;
		if (VEC && rem == 4) return __builtin_nontemporal_load((const j2_v4f *)r);
		j2_v4f v = {0.f, 0.f, 0.f, 0.f};
		v.x = r[0];
		if (rem > 1) v.y = r[1];
		if (rem > 2) v.z = r[2];
		if (rem > 3) v.w = r[3];
		return v;
	};
	unsigned ri = r0;
	RunDesc rd = first, rn = j2_run(runs, r0 + 1 < r1 ? r0 + 1 : r0);
	unsigned left = rd.count;
	unsigned long long t = 0;
	bool over = false;
	while (!over && t < total) {
		for (; left >= (unsigned)J2_NL; left -= J2_NL, t += J2_NL) { // whole batches inside the current run
			j2_v4f v[J2_NL];
#pragma unroll
			for (int j = 0; j < J2_NL; j++) v[j] = load(t + (unsigned)j);
#pragma unroll
			for (int j = 0; j < J2_NL; j++) { a0 += (double)v[j].x; a1 += (double)v[j].y; a2 += (double)v[j].z; a3 += (double)v[j].w; }
		}
		// the batch with the run's last rows (< J2_NL, possibly none: a run that ended with a whole batch is closed here too) and the first rows
		// of what follows
		j2_v4f v[J2_NL];
#pragma unroll
		for (int j = 0; j < J2_NL; j++) // (past the end of the ensemble: the last row again, not added)
			v[j] = load(t + (unsigned)j < total ? t + (unsigned)j : total - 1);
		const unsigned nb = total - t < (unsigned long long)J2_NL ? (unsigned)(total - t) : (unsigned)J2_NL;
		unsigned j0 = 0;
#pragma unroll 1
		do {
			const unsigned n = left < nb - j0 ? left : nb - j0, j1 = j0 + n;
#pragma unroll
			for (int j = 0; j < J2_NL; j++)
				if (__builtin_amdgcn_readfirstlane((int)((unsigned)j >= j0 && (unsigned)j < j1))) { a0 += (double)v[j].x; a1 += (double)v[j].y; a2 += (double)v[j].z; a3 += (double)v[j].w; }
			left -= n; j0 = j1;
			if (left == 0) {
				run_end(rd);
				if (++ri >= r1) { over = true; break; } // (the runs tile the ensemble: nothing is left when the last one ends)
				rd = rn; left = rd.count;
				rn = j2_run(runs, ri + 1 < r1 ? ri + 1 : ri);
			}
		} while (j0 < nb);
		t += nb;
	}
}

// time-domain linear stack of replica slice blockIdx.y (:799-811): (float)((sum_g P[slice Kmax + g]) * (1 / K_c)) to row out_row[slice] of
// out (k_jk_linear's arithmetic, resample.hip, with an output row per slice); K_c = 0: a zero row
__global__ void __launch_bounds__(256) k_jb2_linear(const double *__restrict__ P, unsigned Kmax, size_t N, const unsigned *__restrict__ cnt,
                                                    const unsigned *__restrict__ out_row, float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned s = blockIdx.y, K = cnt[s];
	float *o = out + (size_t)out_row[s] * N;
	if (!K) { o[n] = 0.f; return; }
	const double invK = 1. / (double)K;
	double acc = 0;
	for (unsigned g = 0; g < Kmax; g++) {
		const double v = P[((size_t)s * Kmax + g) * N + n];
		acc = g ? acc + v : v;
	}
	o[n] = (float)(acc * invK);
}

// float outputs of the round's reconstructions x[set][N]: sets [0, nrep) = the replicas' slices (tsPWS_out = (float) x; K_c = 0: zero), then per
// ensemble the plain stack's pair: ICWT(OUT) -> tsPWS, ICWT(ST) -> ls by a FLOAT division by M_b (ts_pws1f_lib.c:233-241)
__global__ void __launch_bounds__(256) k_jb2_epilogue(const double *__restrict__ x, size_t N, unsigned nrep, const unsigned *__restrict__ cnt,
                                                      const unsigned *__restrict__ out_row, float *__restrict__ ls, float *__restrict__ ts,
                                                      float *__restrict__ ts_out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned s = blockIdx.y;
	const double v = x[(size_t)s * N + n];
	if (s < nrep) { ts_out[(size_t)out_row[s] * N + n] = cnt[s] ? (float)v : 0.f; return; }
	const unsigned j = nrep + (s - nrep) / 2; // the plain stack's slice
	if ((s - nrep) & 1u) ls[(size_t)out_row[j] * N + n] = (float)v / (float)cnt[j];
	else ts[(size_t)out_row[j] * N + n] = (float)v;
}

namespace {

struct Ens { unsigned b; size_t f, m; bool unwritten; }; // ensemble with traces: index, first trace, traces; some row of it is never stored

// tables of the whole call: runs and flush destinations of every (ensemble, tile), in that order
struct Tables {
	std::vector<Ens> ens;
	std::vector<RunDesc> runs;      // frow: index into `flush` (of the call)
	std::vector<unsigned> flush;    // destination of a flush as column * KM + group (column C: the plain stack)
	std::vector<size_t> run_ptr;    // runs of (ensemble j, tile q): [run_ptr[j ntile + q], run_ptr[j ntile + q + 1])
	std::vector<size_t> flush_ptr;  // flush destinations of ensemble j: [flush_ptr[j], flush_ptr[j + 1])
};

// runs, column bits and flush destinations of columns [c0, c1) (of W = C [+ 1]) of one ensemble, by the shared rule (column_runs.h)
void build_tile(const char *h_sel, size_t Tn, size_t col0, const Ens &e, unsigned KM, unsigned C, unsigned c0, unsigned c1, unsigned *Kc_out, Tables &T,
                bool &unwritten)
{
	static thread_local ColumnWork work;
	auto sel = [&](unsigned c) { return c < C ? (const unsigned char *)h_sel + (size_t)c * Tn + col0 : nullptr; };
	if (tile_runs(work, e.m, KM, c0, c1, sel, [&](unsigned g, unsigned c) { return c * KM + g; }, e.f, Kc_out, T.runs, T.flush)) unwritten = true;
}

// the tables of a round in one block: trace counts of the nsl slices (doubles) | runs | (ensemble, tile) run ranges | flush rows | counts | output rows
struct J2Tab { size_t mv, run, wg, fl, cnt, row, bytes; };
J2Tab j2_tab(size_t nsl, size_t nruns, size_t nwg, size_t nfl)
{
	TableLayout lay;
	const size_t mv = lay.add<double>(nsl), run = lay.add<RunDesc>(nruns), wg = lay.add<J2Wg>(nwg), fl = lay.add<unsigned>(nfl), cnt = lay.add<unsigned>(nsl),
	             row = lay.add<unsigned>(nsl);
	return {mv, run, wg, fl, cnt, row, lay.bytes};
}

int shared_walk(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const Tables &T, unsigned C, bool main, unsigned ntile, float *d_ls,
                float *d_ts, float *d_ls_out, float *d_ts_out, const unsigned *h_Kc, BatchCall &call, tspws_hip_jk_batch2_stats *stats)
{
	const size_t N = pl->N, nc = pl->ncoef, n = T.ens.size(), budget = tspws_part_budget_bytes();
	hipStream_t st = call.stream();
	const unsigned KM = p->Kmax, W = C + (main ? 1u : 0u);
	int rc;
	void *v;
	// rounds of whole ensembles: the rows, their partials, the plane pairs, the weighted sets / reconstructions / octave buffer of the W (+ 1: the
	// plain stack's ST) sets of an ensemble and the tables within the budget; slices and sets within grid.y, ensembles within grid.z
	const size_t per_ens = std::max({(size_t)W * KM * N * sizeof(double), (size_t)W * KM * pl->npart * sizeof(double2), (size_t)W * 2 * nc * sizeof(double2),
	                                 (size_t)(W + 1) * tspws_inverse_row_bytes(pl)});
	const size_t R = std::max<size_t>(1, std::min<size_t>({budget / per_ens, 65535 / ((size_t)W + 1), 0xffffffffull / ((size_t)W * KM)}));
	auto tab_of = [&](size_t j0, size_t j1) {
		return j2_tab((j1 - j0) * W, T.run_ptr[j1 * ntile] - T.run_ptr[j0 * ntile], (j1 - j0) * ntile, T.flush_ptr[j1] - T.flush_ptr[j0]);
	};
	const std::vector<Round> rounds = whole_ensemble_rounds(n, [&](size_t j0, size_t j1) { return j1 - j0 <= R && tab_of(j0, j1).bytes <= budget; });
	size_t max_ne = 0, max_tab = 0;
	for (const Round &r : rounds) {
		max_ne = std::max(max_ne, r.j1 - r.j0);
		max_tab = std::max(max_tab, tab_of(r.j0, r.j1).bytes);
	}
	if ((size_t)W * KM > 0xffffffffull || max_ne * W * KM > 0xffffffffull) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: more than 2^32 partial-stack rows in a round");
	const size_t max_sl = max_ne * W, max_sets = max_ne * (W + (main ? 1u : 0u));
	if ((rc = scratch(pl, SCR_J2P, max_sl * KM * N * sizeof(double), &v))) return rc;
	double *rows = (double *)v;
	if ((rc = scratch(pl, SCR_PART, std::max<size_t>(1, max_sl * KM * pl->npart) * sizeof(double2), &v))) return rc;
	double2 *part = (double2 *)v;
	if ((rc = scratch(pl, SCR_J2ST, max_sl * 2 * nc * sizeof(double2), &v))) return rc;
	double2 *STr = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWY, max_sets * nc * sizeof(double2), &v))) return rc;
	double2 *OUT = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWX, max_sets * N * sizeof(double), &v))) return rc;
	double *xr = (double *)v;
	const bool fuse = tspws_fused_forward(pl);
	const bool vec = (ld % 4 == 0) && (((uintptr_t)d_x & 15) == 0);
	const unsigned nbx = (unsigned)((N + 1023) / 1024), nb256 = (unsigned)((N + 255) / 256);
	const int mode = tspws_weight_mode(p->wu, p->unbiased, KM);

	for (const Round &r : rounds) {
		const size_t ne = r.j1 - r.j0, nrep = ne * C, nsl = ne * W, nsets = nrep + (main ? 2 * ne : 0), nrows = nsl * KM;
		const size_t q0 = T.run_ptr[r.j0 * ntile], nruns = T.run_ptr[r.j1 * ntile] - q0, f0 = T.flush_ptr[r.j0];
		stats->rounds++;
		stats->rows += (unsigned)nrows;
		// the round's tables (here the counts are the round's own: the bound holds with equality)
		const J2Tab o = tab_of(r.j0, r.j1);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: table bound"); // (cannot happen)
		char *blob = call.block(o.bytes), *tab;
		double *Mv = (double *)(blob + o.mv);
		RunDesc *hr = (RunDesc *)(blob + o.run);
		J2Wg *hw = (J2Wg *)(blob + o.wg);
		unsigned *hfl = (unsigned *)(blob + o.fl), *hcnt = (unsigned *)(blob + o.cnt), *hrow = (unsigned *)(blob + o.row);
		bool unwritten = false;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = T.ens[j];
			const size_t je = j - r.j0;
			unwritten |= e.unwritten;
			for (unsigned c = 0; c < C; c++) { // slice je C + c: replica c; K_c = 0 weighs (zero) stacks with M = 1
				const unsigned K = h_Kc[(size_t)e.b * C + c];
				Mv[je * C + c] = (double)std::max(K, 1u); hcnt[je * C + c] = K; hrow[je * C + c] = (unsigned)((size_t)e.b * C + c);
			}
			if (main) { Mv[nrep + je] = (double)e.m; hcnt[nrep + je] = (unsigned)e.m; hrow[nrep + je] = e.b; }
			for (unsigned q = 0; q < ntile; q++) {
				hw[je * ntile + q].run0 = (unsigned)(T.run_ptr[j * ntile + q] - q0);
				hw[je * ntile + q].run1 = (unsigned)(T.run_ptr[j * ntile + q + 1] - q0);
			}
			for (size_t k = T.flush_ptr[j]; k < T.flush_ptr[j + 1]; k++) { // row of (column, group): the column's slice, Kmax rows each
				const unsigned c = T.flush[k] / KM, g = T.flush[k] % KM;
				hfl[k - f0] = (unsigned)(((c < C ? je * C + c : nrep + je)) * KM + g);
			}
		}
		for (size_t k = 0; k < nruns; k++) { hr[k] = T.runs[q0 + k]; hr[k].frow = (unsigned)(T.runs[q0 + k].frow - f0); }
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const double *d_Mv = (const double *)(tab + o.mv);
		const RunDesc *d_runs = (const RunDesc *)(tab + o.run);
		const J2Wg *d_wg = (const J2Wg *)(tab + o.wg);
		const unsigned *d_fl = (const unsigned *)(tab + o.fl), *d_cnt = (const unsigned *)(tab + o.cnt), *d_row = (const unsigned *)(tab + o.row);

		// the walk: every ensemble's traces once
		if (unwritten) HIP_TRY(hipMemsetAsync(rows, 0, nrows * N * sizeof(double), st));
		const dim3 grid(nbx, ntile, (unsigned)ne);
		if (vec) hipLaunchKernelGGL(k_jb2_rows_walk<true>, grid, dim3(256), 0, st, d_x, ld, N, d_runs, d_wg, d_fl, rows);
		else hipLaunchKernelGGL(k_jb2_rows_walk<false>, grid, dim3(256), 0, st, d_x, ld, N, d_runs, d_wg, d_fl, rows);

		// finish: one slice of Kmax rows per column (finish_replicas of resample.hip over every column of every ensemble)
		FuseOut fz;
		fz.accST = STr; fz.accPS = STr + nc; fz.stride = 2 * nc; fz.tps = KM;
		if ((rc = tspws_forward_parts<double>(pl, rows, nrows, N, part, st, fuse ? &fz : nullptr, ScaleRange()))) return rc;
		FuseOut fj = fz; // slice j went straight into its ST / PS planes
		tspws_launch_accumulate(pl, (const double2 *)part, KM, STr, STr + nc, 1, &fj, 1, st, (unsigned)nsl, (size_t)KM * pl->npart, 2 * nc, nullptr, nullptr, ScaleRange());
		tspws_weight_batched(pl, OUT, (const double2 *)STr, (const double2 *)STr + nc, mode, (double)KM, p->wu, d_Mv, (unsigned)nrep, nc, 2 * nc, st);
		hipLaunchKernelGGL(k_jb2_linear, dim3(nb256, (unsigned)nrep), dim3(256), 0, st, (const double *)rows, KM, N, d_cnt, d_row, d_ls_out);
		if (main) { // the plain stacks: (OUT, ST) pairs behind the replicas' sets
			const double2 *STm = STr + nrep * 2 * nc;
			tspws_weight_batched(pl, OUT + nrep * nc, STm, STm + nc, mode, (double)KM, p->wu, d_Mv + nrep, (unsigned)ne, 2 * nc, 2 * nc, st);
			HIP_TRY(hipMemcpy2DAsync(OUT + nrep * nc + nc, 2 * nc * sizeof(double2), STm, 2 * nc * sizeof(double2), nc * sizeof(double2), ne, hipMemcpyDeviceToDevice, st));
		}
		if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nsets, xr, (void *)st))) return rc;
		hipLaunchKernelGGL(k_jb2_epilogue, dim3(nb256, (unsigned)nsets), dim3(256), 0, st, (const double *)xr, N, (unsigned)nrep, d_cnt, d_row, d_ls, d_ts, d_ts_out);
	}
	return 0;
}

} // namespace

// The shared walk over the ensembles list[0 .. n) of a batch (indices into h_first, ascending; every one two-stage, with traces; column
// h_first[b] - h_first[0] of h_sel[C][Tn] is the first of ensemble b): host tables in one pass over the selection, then rounds of whole ensembles.
// Ensemble b writes rows b * C + c of the replica outputs and of h_mtr_out and, with `main`, row b of d_ls / d_ts; stats: rounds and rows are
// counted up.  The work goes to the stream of the caller's BatchCall, which also owns the uploads' host sources.  (Also what
// tspws_hip_subsample_batch runs for its two-stage ensembles, sub_batch.hip.)
int tspws_jb2_shared(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, const unsigned *list, size_t n, const char *h_sel,
                     size_t Tn, unsigned C, bool main, float *d_ls, float *d_ts, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, BatchCall &call,
                     tspws_hip_jk_batch2_stats *stats)
{
	const unsigned KM = p->Kmax, W = C + (main ? 1u : 0u), ntile = (W + J2_W - 1) / J2_W;
	Tables T;
	T.run_ptr.push_back(0);
	T.flush_ptr.push_back(0);
	for (size_t k = 0; k < n; k++) {
		const unsigned b = list[k];
		Ens e;
		e.b = b; e.f = h_first[b]; e.m = h_first[b + 1] - e.f; e.unwritten = false;
		for (unsigned q = 0; q < ntile; q++) {
			build_tile(h_sel, Tn, e.f - h_first[0], e, KM, C, q * J2_W, std::min(W, (q + 1) * J2_W), h_mtr_out + (size_t)b * C, T, e.unwritten);
			T.run_ptr.push_back(T.runs.size());
		}
		T.flush_ptr.push_back(T.flush.size());
		T.ens.push_back(e);
		if (T.flush.size() > 0xfffffff0ull) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: more than 2^32 partial-stack rows");
	}
	return shared_walk(pl, p, d_x, ld, T, C, main, ntile, d_ls, d_ts, d_ls_out, d_ts_out, h_mtr_out, call, stats);
}

extern "C" int tspws_hip_jackknife_batch_two_stage(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                                                   const char *h_sel, unsigned C, float *d_ls, float *d_ts, float *d_ls_out, float *d_ts_out,
                                                   unsigned *h_mtr_out, void *s)
{
	// (the checks that need no plan come first: a host without a device can see every one of them refuse)
	if (!p || !h_first) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: NULL");
	if (!B || !C) return pl ? 0 : fail(TSPWS_E_ARG, "jackknife_batch_two_stage: NULL");
	if (!h_sel || !d_ls_out || !d_ts_out || !h_mtr_out) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: NULL");
	if (!d_ls != !d_ts) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: exactly one of the main outputs is NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: decreasing ensemble offsets");
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m && !is_two_stage(p, m))
			return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: single-stage parameters for an ensemble (tspws_hip_jackknife_batch takes those)");
		if (m > 0xfffffff0ull) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: more than 2^32 traces in an ensemble");
	}
	if (!pl) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: NULL");
	const size_t N = pl->N, Tn = h_first[B] - h_first[0];
	if (Tn && !d_x) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: NULL traces");
	if (Tn && ld < N) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: row stride below the trace length");
	const bool main = d_ls != nullptr;
	const unsigned KM = p->Kmax, W = C + (main ? 1u : 0u), ntile = (W + J2_W - 1) / J2_W;
	if ((size_t)C + 2 > 65535 || (size_t)W * KM > 0xffffffffull) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage: too many columns (C + 2 <= 65535, (C + 1) Kmax < 2^32)");
	HIP_TRY(hipSetDevice(pl->device));
	hipStream_t st = S_(s);
	int rc;
	std::vector<unsigned> nonempty;
	for (unsigned b = 0; b < B; b++) if (h_first[b + 1] > h_first[b]) nonempty.push_back(b);
	pl->jk_batch2_stats = tspws_hip_jk_batch2_stats();
	pl->jk_batch2_stats.empty = B - (unsigned)nonempty.size();
	pl->jk_batch2_stats.tiles = ntile;
	BatchCall call(st);
	if (nonempty.size() == 1) {
		// one ensemble: the single call, with its columns of the selection
		const unsigned b = nonempty[0];
		const size_t f = h_first[b], m = h_first[b + 1] - f;
		const char *sel = ensemble_selection(call, h_sel, C, Tn, f - h_first[0], m);
		pl->jk_batch2_stats.looped = 1;
		float *lo = d_ls_out + (size_t)b * C * N, *to = d_ts_out + (size_t)b * C * N;
		if (main) rc = tspws_hip_stack_jackknife(pl, p, d_x + f * ld, ld, m, d_ls + (size_t)b * N, d_ts + (size_t)b * N, sel, C, lo, to, h_mtr_out + (size_t)b * C, s);
		else rc = tspws_hip_jackknife(pl, p, d_x + f * ld, ld, m, sel, C, lo, to, h_mtr_out + (size_t)b * C, s);
		if (rc) return rc;
	} else if (nonempty.size() > 1) {
		pl->jk_batch2_stats.shared = (unsigned)nonempty.size();
		if ((rc = tspws_jb2_shared(pl, p, d_x, ld, h_first, nonempty.data(), nonempty.size(), h_sel, Tn, C, main, d_ls, d_ts, d_ls_out, d_ts_out, h_mtr_out, call,
		                           &pl->jk_batch2_stats))) return rc;
	}
	// empty ensembles: zero rows, zero counts
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] == h_first[b]) std::fill_n(h_mtr_out + (size_t)b * C, C, 0u);
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls_out, (size_t)C * N}, {d_ts_out, (size_t)C * N}, {d_ls, N}, {d_ts, N}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

extern "C" int tspws_hip_jackknife_batch_two_stage_stats(const tspws_hip_plan *pl, tspws_hip_jk_batch2_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "jackknife_batch_two_stage_stats: NULL");
	*stats = pl->jk_batch2_stats;
	return 0;
}
