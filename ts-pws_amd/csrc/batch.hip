// batch.hip -- many ensembles of the same trace length in one call (tspws_hip_stack_batch).
// Reference citations are relative to the reference project's src/ directory.
//
// The reference stacks one ensemble per run; its workload is many station pairs, each a small ensemble of daily correlations.  One call
// per small ensemble is a handful of launches of 5-40 us that never reach the engines that fill the GPU.  This unit stacks B ensembles
// [first[b], first[b+1]) of one trace array in one call, every ensemble by the rules of tspws_hip_stack (stage rule, weights, epilogue):
//   single-stage  the ensembles' traces go through ONE many-trace pass (forward.hip: tl_pass_*, engine by the TOTAL trace count):
//                 every ensemble starts a fresh 64-trace block, its traces are gathered into the first lanes of its blocks
//                 (k_batch_gather; idle lanes are zero traces, which add nothing to either stack), the pass leaves one plane pair per
//                 block and per-trace partials, and k_accumulate_parts adds each ensemble's blocks / traces into its own ST / PS and
//                 writes its weighted coefficients with K = M = M_b (runs of equal-sized ensembles share a launch: grid.y).
//                 An ensemble that straddles two batches of the pass keeps accumulating (zero_first on its first segment only).
//   two-stage     ONE streaming pass writes the Kmax partial-stack rows of every ensemble (tspws_run_chunks over a table of row ranges:
//                 row (b, g) = the traces i of ensemble b with floor(i Kmax / M_b) == g, partial_linear_stacks :866-881); the rows
//                 go through the few-trace forward kernels as one batch and k_accumulate_parts stacks each ensemble's Kmax rows
//                 (grid.y = ensemble, weights with K = Kmax and the ensemble's own M_b).
//   finish        per round of stacks: one batched tspws_hip_inverse of the (OUT, ST) pairs, k_batch_epilogue with each row's M_b.
// Rounds keep every scratch block whose size grows with the ensembles -- per-stack sets, reconstructions, the inverse's octave buffer, the
// rows, their partials and the streaming pass's chunk sums -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble.
//   band finish   tspws_hip_stack_batch_bands: the same passes and rounds, but every round's (OUT, ST) pairs go through the band rows of
//                 the inverse (inverse.hip: tspws_inverse_bands_run) -- R float rows per output and, on request, their envelopes, written
//                 by the combining kernel; no FP64 reconstructions, no epilogue.  Ensembles that go to one single call each get their pair
//                 from the public pieces (looped_bands).
// Batches that the many-trace rule would not take as a whole, and a batch with a single ensemble of its kind, fall back to one
// tspws_hip_stack per ensemble.  tspws_hip_stack_batch_stats tells which way the last call's ensembles went.
#include "tspws_internal.h"
#include "batch_kernels.h"
#include "batch_host.h"

#define is_two_stage tspws_is_two_stage

// k_epilogue for a round of stacks: rows 2j / 2j + 1 of x are ICWT(OUT) / ICWT(ST) of stack j = blockIdx.y; its outputs go to row[j] of
// ls / ts, ls by a FLOAT division by the stack's trace count (ts_pws1f_lib.c:233-241)
__global__ void __launch_bounds__(256) k_batch_epilogue(const double *__restrict__ x, size_t N, const unsigned *__restrict__ row,
                                                        const unsigned *__restrict__ cnt, float *__restrict__ ls, float *__restrict__ ts)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const unsigned j = blockIdx.y;
	const size_t o = (size_t)row[j] * N + n;
	ls[o] = (float)x[(2 * (size_t)j + 1) * N + n] / (float)cnt[j];
	ts[o] = (float)x[2 * (size_t)j * N + n];
}

namespace {

// the chunk tables of the two-stage rounds: sources of tspws_run_chunks' uploads like the blocks of the BatchCall, but typed vectors of the
// caller's -- the entry point declares them BEFORE its BatchCall, so that they are destroyed after its destructor has waited for the stream
struct HostTables {
	std::vector<std::vector<Chunk>> chunks;
	std::vector<std::vector<unsigned>> row_first;
};

// stacks of one round: [nr][OUT | ST] (the inverse's rows) and [nr][PS | unused] (ST and PS of a stack share one stride), reconstructions
struct RoundBufs { double2 *Y, *PS; double *x; };

// the band-limited finish of tspws_hip_stack_batch_bands (nullptr: tspws_hip_stack_batch's own): the band table and the envelope outputs
struct BandFinish { const tspws_band *bands; unsigned R; float *ls_env, *ts_env; };

int round_bufs(tspws_hip_plan *pl, size_t nr, RoundBufs *b, const BandFinish *bf = nullptr)
{
	const size_t nc = pl->ncoef;
	void *v;
	int rc;
	if ((rc = scratch(pl, SCR_BY, 4 * nr * nc * sizeof(double2), &v))) return rc;
	b->Y = (double2 *)v; b->PS = b->Y + 2 * nr * nc;
	b->x = nullptr;
	if (bf) return 0; // (the band finish keeps no FP64 reconstructions)
	if ((rc = scratch(pl, SCR_BX, 2 * nr * (size_t)pl->N * sizeof(double), &v))) return rc;
	b->x = (double *)v;
	return 0;
}

// stacks per round: every per-stack scratch block within the parts budget -- the sets (SCR_BY: OUT, ST, PS and an unused one), the two rows of
// the inverse (its sets, reconstructions and octave buffer) and `extra` bytes per stack of the caller's own --, at most 65535 (grid.y)
size_t round_size(const tspws_hip_plan *pl, size_t n, size_t extra)
{
	const size_t r = tspws_part_budget_bytes() / std::max({4 * pl->ncoef * sizeof(double2), 2 * tspws_inverse_row_bytes(pl), extra});
	return std::max<size_t>(1, std::min<size_t>({r, n, 65535}));
}

// inverses + epilogue of stacks [j0, j0 + nr) of a list whose output rows / trace counts are the device tables d_row / d_cnt
// bf: the band rows of every pair instead, floats straight from the combining kernel (d_row NULL: the stacks are the output rows row0 .. with cnt0 traces)
int round_finish(tspws_hip_plan *pl, const RoundBufs &b, unsigned nr, const unsigned *d_row, const unsigned *d_cnt, float *d_ls, float *d_ts, hipStream_t st,
                 const BandFinish *bf, unsigned row0 = 0, unsigned cnt0 = 1)
{
	int rc;
	if (bf) {
		BandOut out;
		out.ts = d_ts; out.ls = d_ls; out.ts_env = bf->ts_env; out.ls_env = bf->ls_env;
		out.d_row = d_row; out.d_cnt = d_cnt; out.row0 = row0; out.cnt0 = cnt0;
		return tspws_inverse_bands_run(pl, b.Y, 2 * (size_t)nr, bf->bands, bf->R, out, st, &pl->stack_bands_stats.finish_batches, &pl->stack_bands_stats.scales);
	}
	if ((rc = tspws_hip_inverse(pl, (const double *)b.Y, 2 * (size_t)nr, b.x, (void *)st))) return rc;
	hipLaunchKernelGGL(k_batch_epilogue, dim3((pl->N + 255) / 256, nr), dim3(256), 0, st, (const double *)b.x, (size_t)pl->N, d_row, d_cnt, d_ls, d_ts);
	return 0;
}

// Single-stage ensembles `ens` (all with traces) through one many-trace pass.
int batch_single(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *first, const std::vector<unsigned> &ens,
                 size_t total, float *d_ls, float *d_ts, BatchCall &call, const BandFinish *bf)
{
	const size_t N = pl->N, nc = pl->ncoef, n = ens.size();
	hipStream_t st = call.stream();
	int rc;
	void *v;
	// block layout of every ensemble (the whole call), the gather table of its slots, output rows and trace counts
	std::vector<size_t> blk0(n + 1);
	for (size_t j = 0; j < n; j++) blk0[j + 1] = blk0[j] + (first[ens[j] + 1] - first[ens[j]] + 63) / 64;
	const size_t nslots = blk0[n] * 64;
	TableLayout lay;
	const size_t o_src = lay.add<long long>(nslots), o_row = lay.add<unsigned>(n), o_cnt = lay.add<unsigned>(n);
	char *blob = call.block(lay.bytes), *tab;
	long long *src = (long long *)(blob + o_src);
	unsigned *row = (unsigned *)(blob + o_row), *cnt = (unsigned *)(blob + o_cnt);
	for (size_t j = 0; j < n; j++) {
		const size_t f = first[ens[j]], m = first[ens[j] + 1] - f;
		for (size_t i = 0; i < (blk0[j + 1] - blk0[j]) * 64; i++) src[blk0[j] * 64 + i] = i < m ? (long long)(f + i) : -1;
		row[j] = ens[j];
		cnt[j] = (unsigned)m;
	}
	if ((rc = call.upload(pl, SCR_BTAB, blob, lay.bytes, &tab))) return rc;
	const long long *d_src = (const long long *)(tab + o_src);
	const unsigned *d_row = (const unsigned *)(tab + o_row), *d_cnt = (const unsigned *)(tab + o_cnt);

	TlPass P;
	if ((rc = tspws_tl_pass_setup<float>(pl, total, nslots, P))) return rc;
	const TlTable &T = *P.T;
	if ((rc = scratch(pl, SCR_BXG, P.batch * N * sizeof(float), &v))) return rc;
	float *xg = (float *)v;
	const size_t R = round_size(pl, n, 0);
	RoundBufs b;
	if ((rc = round_bufs(pl, R, &b, bf))) return rc;
	for (size_t r0 = 0; r0 < n; r0 += R) {
		const size_t r1 = std::min(n, r0 + R);
		pl->batch_stats.rounds++;
		// the round's blocks in batches of the pass (whole blocks: an ensemble may straddle two batches)
		for (size_t c0 = blk0[r0]; c0 < blk0[r1]; c0 += P.batch / 64) {
			const size_t c1 = std::min(blk0[r1], c0 + P.batch / 64);
			const unsigned nb = (unsigned)((c1 - c0) * 64);
			pl->batch_stats.pass_batches++;
			hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, d_x, ld, d_src + c0 * 64, (unsigned)N, xg);
			if ((rc = tspws_tl_pass_transform<float>(pl, P, xg, N, nb, st))) return rc;
			// the segments of the ensembles in this batch; runs of consecutive segments with the same geometry share one launch
			size_t j = std::upper_bound(blk0.begin(), blk0.end(), c0) - blk0.begin() - 1;
			while (j < r1 && blk0[j] < c1) {
				struct Seg { size_t b0, nblk, ntr; bool head, tail; unsigned m; };
				auto seg = [&](size_t e) {
					Seg s;
					const size_t m = cnt[e], s0 = std::max(blk0[e], c0), s1 = std::min(blk0[e + 1], c1);
					s.b0 = s0; s.nblk = s1 - s0;
					s.ntr = std::min(m, (s1 - blk0[e]) * 64) - (s0 - blk0[e]) * 64;
					s.head = s0 == blk0[e]; s.tail = s1 == blk0[e + 1]; s.m = (unsigned)m;
					return s;
				};
				const Seg a = seg(j);
				size_t k = j + 1;
				while (k < r1 && blk0[k] < c1) {
					const Seg s = seg(k);
					if (s.nblk != a.nblk || s.ntr != a.ntr || s.head != a.head || s.tail != a.tail || (a.tail && s.m != a.m)) break;
					k++;
				}
				const size_t jr = j - r0; // stack of the round
				FuseOut fz;
				fz.accST = P.planes + (a.b0 - c0) * 2 * nc; fz.accPS = fz.accST + nc; fz.stride = 2 * nc; fz.tps = 64; fz.applied = true;
				AccExtra ex;
				ex.y_fz = a.nblk * 2 * nc;
				WeightArgs wa;
				wa.OUT = b.Y + 2 * jr * nc; wa.out_stride = 2 * nc;
				wa.mode = tspws_weight_mode(p->wu, p->unbiased, a.m); wa.K = wa.M = (double)a.m; wa.wu = p->wu;
				const double2 *part = P.part ? P.part + (a.b0 - c0) * 64 * T.npart : nullptr;
				tspws_launch_accumulate(pl, part, (unsigned)a.ntr, b.Y + (2 * jr + 1) * nc, b.PS + 2 * jr * nc, a.head ? 1 : 0, &fz, (unsigned)a.nblk, st,
				                        (unsigned)(k - j), a.nblk * 64 * T.npart, 2 * nc, &T, a.tail ? &wa : nullptr, ScaleRange(), &ex);
				j = k;
			}
		}
		if ((rc = round_finish(pl, b, (unsigned)(r1 - r0), d_row + r0, d_cnt + r0, d_ls, d_ts, st, bf))) return rc;
	}
	return 0;
}

// Two-stage ensembles `ens` (Kmax <= M_b): one streaming pass for all their partial-stack rows, the rows through the few-trace forward.
int batch_two_stage(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *first, const std::vector<unsigned> &ens,
                    size_t total, float *d_ls, float *d_ts, BatchCall &call, HostTables &chunk_tabs, const BandFinish *bf)
{
	const size_t N = pl->N, nc = pl->ncoef, n = ens.size();
	const unsigned K = p->Kmax;
	hipStream_t st = call.stream();
	int rc;
	void *v;
	TableLayout lay;
	const size_t o_row = lay.add<unsigned>(n), o_cnt = lay.add<unsigned>(n), o_mv = lay.add<double>(n);
	char *blob = call.block(lay.bytes), *tab;
	unsigned *row = (unsigned *)(blob + o_row), *cnt = (unsigned *)(blob + o_cnt);
	double *Mv = (double *)(blob + o_mv);
	for (size_t j = 0; j < n; j++) {
		row[j] = ens[j];
		cnt[j] = (unsigned)(first[ens[j] + 1] - first[ens[j]]);
		Mv[j] = (double)cnt[j];
	}
	if ((rc = call.upload(pl, SCR_BTAB, blob, lay.bytes, &tab))) return rc;
	const unsigned *d_row = (const unsigned *)(tab + o_row), *d_cnt = (const unsigned *)(tab + o_cnt);
	const double *d_Mv = (const double *)(tab + o_mv);

	// every ensemble's streaming work items: group g = floor(i Kmax / M_b) of its traces (ts_pws1f_lib.c:876), cut into equal pieces
	const unsigned clen = tspws_chunk_len_for(N, total / n);
	std::vector<Chunk> all;
	std::vector<size_t> ck0(n + 1, 0); // items of ensemble j: [ck0[j], ck0[j + 1]), in group order (row = g)
	for (size_t j = 0; j < n; j++) {
		const size_t f = first[ens[j]], m = cnt[j];
		size_t i = 0;
		while (i < m) {
			const size_t g = (size_t)floor((double)(i * (size_t)K) / (double)m);
			size_t e = i + 1;
			while (e < m && (size_t)floor((double)(e * (size_t)K) / (double)m) == g) e++;
			const size_t cn = e - i, pieces = (cn + clen - 1) / clen, base = cn / pieces, rem = cn % pieces;
			size_t t = f + i;
			for (size_t k = 0; k < pieces; k++) {
				Chunk c; c.t0 = t; c.count = (unsigned)(base + (k < rem ? 1 : 0)); c.row = (unsigned)g;
				all.push_back(c);
				t += c.count;
			}
			i = e;
		}
		ck0[j + 1] = all.size();
	}
	// rounds: the per-stack blocks, the rows (SCR_BP) and their partials (SCR_PART) of at most R ensembles, and the chunk sums of the streaming
	// pass (SCR_CHUNK, N doubles per work item, tspws_chunks_launch) within the budget
	const size_t R = round_size(pl, n, std::max((size_t)K * pl->npart * sizeof(double2), (size_t)K * N * sizeof(double)));
	const size_t ck_cap = std::max<size_t>(1, tspws_part_budget_bytes() / (((N + 3) & ~(size_t)3) * sizeof(double)));
	RoundBufs b;
	if ((rc = round_bufs(pl, R, &b, bf))) return rc;
	if ((rc = scratch(pl, SCR_BP, R * K * N * sizeof(double), &v))) return rc;
	double *rows = (double *)v;
	if ((rc = scratch(pl, SCR_PART, R * K * pl->npart * sizeof(double2), &v))) return rc;
	double2 *part = (double2 *)v;
	for (const Round &rd : whole_ensemble_rounds(n, [&](size_t j0, size_t j1) { return j1 - j0 <= R && ck0[j1] - ck0[j0] <= ck_cap; })) {
		const size_t r0 = rd.j0, r1 = rd.j1, nr = r1 - r0;
		pl->batch_stats.rounds++;
		// chunk table of the round: row jr * K + g = group g of stack jr
		chunk_tabs.chunks.emplace_back(all.begin() + ck0[r0], all.begin() + ck0[r1]);
		chunk_tabs.row_first.emplace_back(nr * K + 1, 0);
		std::vector<Chunk> &ck = chunk_tabs.chunks.back();
		std::vector<unsigned> &rf = chunk_tabs.row_first.back();
		for (size_t jr = 0; jr < nr; jr++)
			for (size_t q = ck0[r0 + jr] - ck0[r0]; q < ck0[r0 + jr + 1] - ck0[r0]; q++) ck[q].row += (unsigned)(jr * K);
		for (size_t q = ck.size(); q-- > 0;) rf[ck[q].row] = (unsigned)q; // (every group has traces: Kmax <= M_b)
		rf[nr * K] = (unsigned)ck.size();
		if ((rc = tspws_run_chunks(pl, d_x, ld, N, ck, rf, (unsigned)(nr * K), rows, N, st, false))) return rc;
		if ((rc = tspws_forward_parts<double>(pl, rows, nr * K, N, part, st, nullptr, ScaleRange()))) return rc;
		WeightArgs wa;
		wa.OUT = b.Y; wa.out_stride = 2 * nc;
		wa.mode = tspws_weight_mode(p->wu, p->unbiased, K); wa.K = (double)K; wa.wu = p->wu; wa.Mv = d_Mv + r0;
		tspws_launch_accumulate(pl, part, K, b.Y + nc, b.PS, 1, nullptr, 0, st, (unsigned)nr, (size_t)K * pl->npart, 2 * nc, nullptr, &wa, ScaleRange());
		if ((rc = round_finish(pl, b, (unsigned)nr, d_row + r0, d_cnt + r0, d_ls, d_ts, st, bf))) return rc;
	}
	return 0;
}

// One ensemble that the batch hands to a single call, for the band finish (tspws_hip_stack writes its floats from inside the inverse): its pair
// of sets from the public pieces -- tspws_hip_stacks_float, or tspws_hip_partial_stacks + tspws_hip_stacks_double, then tspws_hip_weight.
int looped_bands(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t m, unsigned b, float *d_ls, float *d_ts, void *s, const BandFinish *bf)
{
	const size_t N = pl->N, nc = pl->ncoef;
	RoundBufs rb;
	int rc;
	if ((rc = round_bufs(pl, 1, &rb, bf))) return rc;
	double *OUT = (double *)rb.Y, *ST = (double *)(rb.Y + nc), *PS = (double *)rb.PS;
	unsigned K = (unsigned)m;
	if (is_two_stage(p, m)) {
		void *v;
		K = p->Kmax;
		if ((rc = scratch(pl, SCR_BP, (size_t)K * N * sizeof(double), &v))) return rc;
		if ((rc = tspws_hip_partial_stacks(pl, d_x, ld, m, 0, m, K, (double *)v, N, s))) return rc;
		if ((rc = tspws_hip_stacks_double(pl, (const double *)v, K, N, ST, PS, s))) return rc;
	} else if ((rc = tspws_hip_stacks_float(pl, d_x, m, ld, ST, PS, s))) return rc;
	if ((rc = tspws_hip_weight(pl, OUT, ST, PS, K, (unsigned)m, p->wu, p->unbiased, s))) return rc;
	return round_finish(pl, rb, 1, nullptr, nullptr, d_ls, d_ts, S_(s), bf, b, (unsigned)m);
}

// tspws_hip_stack_batch (bf == nullptr) and tspws_hip_stack_batch_bands: the arguments are checked
int stack_batch_run(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B, float *d_ls, float *d_ts, void *s,
                    const BandFinish *bf)
{
	const size_t N = pl->N, NR = bf ? (size_t)bf->R * N : N; // floats per ensemble of an output
	hipStream_t st = S_(s);
	int rc;
	std::vector<unsigned> one, two; // ensembles with traces by stage rule
	size_t n1 = 0, n2 = 0;
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (!m) continue;
		if (is_two_stage(p, m)) { two.push_back(b); n2 += m; }
		else { one.push_back(b); n1 += m; }
	}
	HostTables chunk_tabs; // (before `call`: see HostTables)
	BatchCall call(st);
	pl->batch_stats = tspws_hip_batch_stats();
	pl->batch_stats.empty = B - (unsigned)(one.size() + two.size());
	auto looped = [&](const std::vector<unsigned> &list) { // one tspws_hip_stack per ensemble
		pl->batch_stats.looped += (unsigned)list.size();
		for (unsigned b : list)
			if (int e = bf ? looped_bands(pl, p, d_x + h_first[b] * ld, ld, h_first[b + 1] - h_first[b], b, d_ls, d_ts, s, bf)
			               : tspws_hip_stack(pl, p, d_x + h_first[b] * ld, ld, h_first[b + 1] - h_first[b], d_ls + (size_t)b * N, d_ts + (size_t)b * N, s)) return e;
		return 0;
	};
	if (one.size() > 1 && tspws_many_trace_path(pl, n1)) {
		pl->batch_stats.single_pass = (unsigned)one.size();
		if ((rc = batch_single(pl, p, d_x, ld, h_first, one, n1, d_ls, d_ts, call, bf))) return rc;
	} else if ((rc = looped(one))) return rc;
	if (two.size() > 1) {
		pl->batch_stats.two_stage_pass = (unsigned)two.size();
		if ((rc = batch_two_stage(pl, p, d_x, ld, h_first, two, n2, d_ls, d_ts, call, chunk_tabs, bf))) return rc;
	} else if ((rc = looped(two))) return rc;
	if ((rc = zero_empty_ensembles(h_first, B, st, {{d_ls, NR}, {d_ts, NR}, {bf ? bf->ls_env : nullptr, NR}, {bf ? bf->ts_env : nullptr, NR}}))) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

// what tspws_hip_stack_batch refuses of its traces and offsets (who: the entry point's name in the text)
int batch_args(const char *who, const tspws_hip_plan *pl, const float *d_x, size_t ld, const size_t *h_first, unsigned B)
{
	const std::string w(who);
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, (w + ": decreasing ensemble offsets").c_str());
	const bool any = h_first[B] > h_first[0];
	if (any && !d_x) return fail(TSPWS_E_ARG, (w + ": NULL traces").c_str());
	if (any && ld < pl->N) return fail(TSPWS_E_ARG, (w + ": row stride below the trace length").c_str());
	return 0;
}

} // namespace

extern "C" int tspws_hip_stack_batch(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                                     float *d_ls, float *d_ts, void *s)
{
	if (!pl || !p || !h_first) return fail(TSPWS_E_ARG, "stack_batch: NULL");
	if (!B) return 0;
	if (!d_ls || !d_ts) return fail(TSPWS_E_ARG, "stack_batch: NULL output");
	if (int rc = batch_args("stack_batch", pl, d_x, ld, h_first, B)) return rc;
	HIP_TRY(hipSetDevice(pl->device));
	return stack_batch_run(pl, p, d_x, ld, h_first, B, d_ls, d_ts, s, nullptr);
}

extern "C" int tspws_hip_stack_batch_bands(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                                           const tspws_band *h_bands, unsigned R, float *d_ls, float *d_ts, float *d_ls_env, float *d_ts_env, void *s)
{
	// (the checks that need no plan first)
	if (int rc = tspws_bands_check(pl, h_bands, R, "stack_batch_bands")) return rc;
	if (!d_ls_env != !d_ts_env) return fail(TSPWS_E_ARG, "stack_batch_bands: the two envelope outputs are both NULL or both given");
	if (h_first)
		for (unsigned b = 0; b < B; b++)
			if (h_first[b + 1] < h_first[b]) return fail(TSPWS_E_ARG, "stack_batch_bands: decreasing ensemble offsets");
	if (!pl || !p || !h_first) return fail(TSPWS_E_ARG, "stack_batch_bands: NULL");
	if (!B || !R) return 0;
	if (!h_bands) return fail(TSPWS_E_ARG, "stack_batch_bands: NULL band table");
	if (!d_ls || !d_ts) return fail(TSPWS_E_ARG, "stack_batch_bands: NULL output");
	if (int rc = batch_args("stack_batch_bands", pl, d_x, ld, h_first, B)) return rc;
	HIP_TRY(hipSetDevice(pl->device));
	pl->stack_bands_stats = tspws_hip_stack_bands_stats();
	pl->stack_bands_stats.quadrature = d_ls_env ? 1u : 0u;
	const BandFinish bf = {h_bands, R, d_ls_env, d_ts_env};
	const tspws_hip_batch_stats plain = pl->batch_stats; // (tspws_hip_stack_batch_stats keeps answering for the last tspws_hip_stack_batch call)
	const int rc = stack_batch_run(pl, p, d_x, ld, h_first, B, d_ls, d_ts, s, &bf);
	pl->stack_bands_stats.batch = pl->batch_stats;
	pl->batch_stats = plain;
	return rc;
}

extern "C" int tspws_hip_stack_batch_bands_stats(const tspws_hip_plan *pl, tspws_hip_stack_bands_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "stack_batch_bands_stats: NULL");
	*stats = pl->stack_bands_stats;
	return 0;
}

extern "C" int tspws_hip_stack_batch_stats(const tspws_hip_plan *pl, tspws_hip_batch_stats *stats)
{
	if (!pl || !stats) return fail(TSPWS_E_ARG, "stack_batch_stats: NULL");
	*stats = pl->batch_stats;
	return 0;
}
