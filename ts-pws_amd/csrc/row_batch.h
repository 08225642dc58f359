// row_batch.h -- the rows of many single-stage ensembles in one call: what sub_batch.hip (a row is a 0/1 mask over the traces), boot_batch.hip
// (a count per trace) and weighted_batch.hip (an FP64 weight per trace) share, which is everything but the row's code.
//
// The host matrix of a call is [M][T]: row q says of every trace of the batch how it enters row q of its ensemble.  Ensembles go in rounds:
//   host       rounds of whole ensembles (whole_ensemble_rounds); per round one table block: ensembles | count of every row | what else the
//              finish needs of a row | the codes.  The codes of group g of 8 rows hold one entry per trace j at [bits_off + g m + j], lane
//              q & 7 of it what row q = 8 g + lane says of the trace (pack_columns; lanes past M stay zero)
//   per round  the round's traces are transformed once (tspws_forward_parts, ONE call per stretch of contiguous traces: ensembles left out in
//              between cut a stretch, empty ones do not) into per-trace partials; k_rb_accumulate (coefficient tile x group of 8 rows x
//              ensemble) walks an ensemble's traces in trace order, sums each over its splits, normalises it once and lets the code add it to
//              the register-held stacks of the 8 rows -- the arithmetic of k_accumulate_masked (resample.hip), with the 8 codes of a trace in
//              one wave-uniform entry and every ST / PS plane written exactly once, zero planes included: no memset, no read-modify-write;
//              k_rb_linear (sample tile x row x ensemble): k_sub_linear's float accumulator (ts_pws1f_lib.c:538-542, relative to the reference
//              project's src/); then, per batch of rows that fits, the policy's weight kernel with each row's own count (the mode per row), one
//              tspws_hip_inverse and k_sb_epilogue, which scatters the float rows to [b][m]; then the caller's end-of-round step
// Rounds keep every block that grows with the ensembles -- partials, plane pairs, weighted sets, reconstructions, the inverse's octave buffer,
// tables -- within the parts budget (TSPWS_PART_MB); a round never splits an ensemble, one ensemble alone may exceed it.  Nothing is atomic;
// every output has one writer and every sum a fixed order.
//
// A policy P states the code of a row (a unit defines one, next to its entry points):
//   Entry, Value     the 8 codes of a trace in the table; one element of the host matrix.  put(entry, lane, value) packs one
//   SPARE            zero entries behind a round's codes (CODES_AHEAD reads up to 3 past an ensemble's last)
//   Codes, fetch, add(codes, m, st, ps, a, u)   k_rb_accumulate: the 8 codes of a trace, wave-uniform, and what code m adds to the stacks of row m.
//                    CODES_AHEAD: fetched without a branch at the top of the four-trace block, not under the trace's bound in the add loop
//   Lane, Code, code(x, lane), add(acc, code, x)  k_rb_linear: an entry as lanes (a mask byte is one lane), one row's code of a trace from its
//                    lane, and its addend.  LOAD_ALL: every trace is loaded (clamped to the last one), not only those whose code is not zero
//   Rows, Row        the rows of a round to the kernels: kc[r], the count of row r (0: a zero row), total(r), the divisor of its linear stack, and
//                    (Row not void) one more record per row, h_rows[b M + q] on the host
//   launch_weight    the weight kernel of a finish batch
//   NAME, ROWS       the call and its rows in messages
#pragma once

#include "batch_kernels.h"
#include "batch_host.h"

#include <type_traits>

// the rows of the mask and count policies: a row is its K
struct KRows {
	const unsigned *kc;
	static KRows at(const unsigned *kc, const void *) { return {kc}; }
	__device__ double total(size_t r) const { return (double)kc[r]; }
};
static inline void launch_sb_weight(dim3 grid, hipStream_t st, double2 *OUT, const double2 *planes, size_t nc, const KRows &rows, size_t r0, const t_tsPWS *p)
{
	hipLaunchKernelGGL(k_sb_weight, grid, dim3(256), 0, st, OUT, planes, nc, rows.kc, r0, p->wu, p->unbiased);
}

// ST / PS planes of the rows 8 g .. 8 g + 7 (g = g0 + blockIdx.y) of ensemble blockIdx.z of the round, one thread per coefficient (the
// geometry of k_accumulate_masked: 256-coefficient blocks by acc_off).  Row r = blockIdx.z M + row: planes[r][ST | PS], 2 ncoef apart.
template <class P>
static __global__ void __launch_bounds__(256) k_rb_accumulate(const double2 *__restrict__ part, size_t npart, const ScaleDesc *__restrict__ sc, unsigned S,
                                                               size_t ncoef, const SbEns *__restrict__ ens, const typename P::Entry *__restrict__ tab, unsigned M,
                                                               unsigned g0, double2 *__restrict__ planes)
{
	const unsigned lo = find_block_scale(sc, S, blockIdx.x, false);
	const unsigned Ns = sc[lo].Ns, nsplit = sc[lo].nsplit;
	const unsigned k = (blockIdx.x - sc[lo].acc_off) * 256 + threadIdx.x;
	if (k >= Ns) return;
	const size_t i = sc[lo].coef_off + k;
	const SbEns e = ens[blockIdx.z];
	const unsigned g = g0 + blockIdx.y, m0 = g * 8u, nm = (M - m0) < 8u ? (M - m0) : 8u, ntr = e.m;
	const typename P::Entry *tb = tab + e.bits_off + (size_t)g * ntr;
	const double2 *p0 = part + (size_t)e.part0 * npart + sc[lo].part_off + k;
	double2 st[8], ps[8];
#pragma unroll
	for (int m = 0; m < 8; m++) { st[m] = make_double2(0, 0); ps[m] = make_double2(0, 0); }
	for (unsigned b0 = 0; b0 < ntr; b0 += 4) { // four traces at a time: their loads are independent, the additions stay in trace order
		double2 a[4], u[4];
		typename P::Codes c[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			a[j] = make_double2(0, 0);
			if (b0 + (unsigned)j < ntr) a[j] = p0[(size_t)(b0 + (unsigned)j) * npart];
			if (P::CODES_AHEAD) c[j] = P::fetch(tb + b0 + (unsigned)j); // (the address depends on the block and the loop alone)
		}
		for (unsigned sp = 1; sp < nsplit; sp++) {
			double2 t[4];
#pragma unroll
			for (int j = 0; j < 4; j++) t[j] = (b0 + (unsigned)j < ntr) ? p0[(size_t)(b0 + (unsigned)j) * npart + (size_t)sp * Ns] : make_double2(0, 0);
#pragma unroll
			for (int j = 0; j < 4; j++) { a[j].x += t[j].x; a[j].y += t[j].y; }
		}
#pragma unroll
		for (int j = 0; j < 4; j++) { u[j] = make_double2(0, 0); add_unit_phasor(u[j], a[j]); }
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (b0 + (unsigned)j < ntr) {
				if (!P::CODES_AHEAD) c[j] = P::fetch(tb + b0 + (unsigned)j);
#pragma unroll
				for (int m = 0; m < 8; m++) P::add(c[j], m, st[m], ps[m], a[j], u[j]);
			}
		}
	}
	double2 *o = planes + ((size_t)blockIdx.z * M + m0) * 2 * ncoef + i;
#pragma unroll
	for (int m = 0; m < 8; m++)
		if ((unsigned)m < nm) { o[(size_t)m * 2 * ncoef] = st[m]; o[(size_t)m * 2 * ncoef + ncoef] = ps[m]; }
}

// time-domain linear stack of row q0 + blockIdx.y of ensemble blockIdx.z: the reference's FLOAT accumulator over the traces in trace order
// (ts_pws1f_lib.c:538-542) with the code's addend, then the float scale 1 / total (:579-583) -- k_sub_linear (resample.hip) per (row,
// ensemble); a row whose count is 0: a zero row
template <class P>
static __global__ void __launch_bounds__(256) k_rb_linear(const float *__restrict__ x, size_t ld, size_t N, const SbEns *__restrict__ ens,
                                                           const typename P::Entry *__restrict__ tab, const typename P::Rows rows, unsigned M, unsigned q0,
                                                           float *__restrict__ out)
{
	const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (n >= N) return;
	const SbEns e = ens[blockIdx.z];
	const unsigned q = q0 + blockIdx.y, lane = q & 7u;
	const size_t r = (size_t)blockIdx.z * M + q;
	float *o = out + ((size_t)e.row * M + q) * N;
	if (!rows.kc[r]) { o[n] = 0.f; return; }
	constexpr size_t LANES = sizeof(typename P::Entry) / sizeof(typename P::Lane); // lanes an entry apart: the row's codes
	const typename P::Lane *row = (const typename P::Lane *)tab + (e.bits_off + (size_t)(q >> 3) * e.m) * LANES + (LANES > 1 ? lane : 0u);
	const float *xe = x + (size_t)e.t0 * ld + n;
	const size_t mtr = e.m;
	float acc = 0.f;
	for (size_t i0 = 0; i0 < mtr; i0 += 8) { // eight rows' loads in flight; the additions keep the trace order
		float v[8];
		typename P::Code c[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const bool in = i0 + (size_t)j < mtr;
			const size_t t = in || !P::LOAD_ALL ? i0 + (size_t)j : mtr - 1;
			if (P::LOAD_ALL) v[j] = xe[t * ld]; // (no branch around a load)
			c[j] = in ? P::code(row[t * LANES], lane) : typename P::Code(0); // (wave-uniform)
			if (!P::LOAD_ALL) v[j] = c[j] != 0 ? xe[t * ld] : 0.f;
		}
#pragma unroll
		for (int j = 0; j < 8; j++) acc = P::add(acc, c[j], v[j]);
	}
	o[n] = acc * (float)(1. / rows.total(r));
}

struct Ens { unsigned b; size_t f, m; }; // ensemble with traces: index, first trace, traces

// the tables of a round in one block: ensembles | count of every row | the rows' records | codes
struct RowTab { size_t ens, kc, rows, codes, bytes; };
template <class P>
static inline RowTab row_tab(size_t ne, size_t nrows, size_t ncodes)
{
	TableLayout lay;
	RowTab o{};
	o.ens = lay.add<SbEns>(ne);
	o.kc = lay.add<unsigned>(nrows);
	if constexpr (!std::is_void_v<typename P::Row>) o.rows = lay.add<typename P::Row>(nrows);
	o.codes = lay.add<typename P::Entry>(ncodes + P::SPARE);
	o.bytes = lay.bytes;
	return o;
}

// columns [col0, col0 + m) of h[M][T] as the entries of one ensemble (dst: zero so far)
template <class P>
static inline void pack_columns(typename P::Entry *dst, const typename P::Value *h, unsigned M, size_t T, size_t col0, size_t m)
{
	for (unsigned q = 0; q < M; q++) {
		const typename P::Value *row = h + (size_t)q * T + col0;
		typename P::Entry *d = dst + (size_t)(q >> 3) * m;
		for (size_t i = 0; i < m; i++) P::put(d[i], q & 7u, row[i]);
	}
}

// the ensembles E of the batch in rounds.  rows: the call's host matrix h[M][Tn] (and h_rows); h_Kc[b M + q]: the count of every row;
// round_end(d_ens, d_kc, ne): enqueued behind the finish of every round
template <class P, class RoundEnd>
static int row_batch_rounds(tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, size_t first0, const std::vector<Ens> &E, unsigned M, const P &rows,
                            size_t Tn, float *d_ls_out, float *d_ts_out, const unsigned *h_Kc, unsigned &nrounds, BatchCall &call, RoundEnd round_end)
{
	const size_t N = pl->N, nc = pl->ncoef, n = E.size(), budget = tspws_part_budget_bytes();
	const std::string name = P::NAME;
	hipStream_t st = call.stream();
	const unsigned ng = (M + 7) / 8;
	int rc;
	void *v;
	// rounds of whole ensembles: the partials of their traces, a plane pair per (ensemble, row) and the tables within the budget; ensembles
	// within grid.z, partial indices and rows within 32 bits
	std::vector<size_t> tr0(n + 1, 0); // traces in front of ensemble j
	for (size_t j = 0; j < n; j++) tr0[j + 1] = tr0[j] + E[j].m;
	auto tab_of = [&](size_t j0, size_t j1) { return row_tab<P>(j1 - j0, (j1 - j0) * M, (tr0[j1] - tr0[j0]) * ng); };
	const std::vector<Round> rounds = whole_ensemble_rounds(n, [&](size_t j0, size_t j1) {
		const size_t ne = j1 - j0, nt = tr0[j1] - tr0[j0];
		return !(ne > 65535 || ne * M > 0xfffffff0ull || nt > 0xfffffff0ull || nt * pl->npart * sizeof(double2) > budget || ne * M * 2 * nc * sizeof(double2) > budget ||
		         tab_of(j0, j1).bytes > budget);
	});
	size_t max_ntr = 0, max_ne = 0, max_tab = 0;
	for (const Round &r : rounds) {
		max_ntr = std::max(max_ntr, tr0[r.j1] - tr0[r.j0]);
		max_ne = std::max(max_ne, r.j1 - r.j0);
		max_tab = std::max(max_tab, tab_of(r.j0, r.j1).bytes);
	}
	if (max_ntr > 0xfffffff0ull || max_ne * M > 0xfffffff0ull) return fail(TSPWS_E_ARG, (name + ": more than 2^32 traces or " + P::ROWS + " in one ensemble").c_str());
	// rows per finish batch
	const size_t RB = even_rows_per_batch(budget, tspws_inverse_row_bytes(pl), max_ne * M);
	// (SCR_SBPL: the plane pairs of whichever unit is running; none keeps a pointer across calls)
	if ((rc = scratch(pl, SCR_PART, std::max<size_t>(2, max_ntr) * pl->npart * sizeof(double2), &v))) return rc;
	double2 *part = (double2 *)v;
	if ((rc = scratch(pl, SCR_SBPL, max_ne * M * 2 * nc * sizeof(double2), &v))) return rc;
	double2 *planes = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWY, RB * nc * sizeof(double2), &v))) return rc;
	double2 *OUT = (double2 *)v;
	if ((rc = scratch(pl, SCR_ROWX, RB * N * sizeof(double), &v))) return rc;
	double *xr = (double *)v;
	const unsigned nb256 = (unsigned)((N + 255) / 256);

	for (const Round &r : rounds) {
		const size_t ne = r.j1 - r.j0, nrows = ne * M;
		nrounds++;
		// the round's tables (here the counts are the round's own: the bound holds with equality)
		const RowTab o = tab_of(r.j0, r.j1);
		if (o.bytes > max_tab) return fail(TSPWS_E_ARG, (name + ": table bound").c_str()); // (cannot happen)
		char *blob = call.block(o.bytes), *tab;
		SbEns *he = (SbEns *)(blob + o.ens);
		size_t t = 0;
		for (size_t j = r.j0; j < r.j1; j++) {
			const Ens &e = E[j];
			SbEns d;
			d.t0 = e.f; d.bits_off = t * ng; d.m = (unsigned)e.m; d.part0 = (unsigned)t; d.row = e.b; d.pad = 0;
			he[j - r.j0] = d;
			memcpy((unsigned *)(blob + o.kc) + (j - r.j0) * (size_t)M, h_Kc + (size_t)e.b * M, (size_t)M * sizeof(unsigned));
			if constexpr (!std::is_void_v<typename P::Row>)
				memcpy((typename P::Row *)(blob + o.rows) + (j - r.j0) * (size_t)M, rows.h_rows + (size_t)e.b * M, (size_t)M * sizeof(typename P::Row));
			pack_columns<P>((typename P::Entry *)(blob + o.codes) + d.bits_off, rows.h, M, Tn, e.f - first0, e.m);
			t += e.m;
		}
		if ((rc = call.upload(pl, SCR_BTAB, blob, o.bytes, &tab, max_tab))) return rc;
		const SbEns *d_ens = (const SbEns *)(tab + o.ens);
		const typename P::Entry *d_codes = (const typename P::Entry *)(tab + o.codes);
		const typename P::Rows d_rows = P::Rows::at((const unsigned *)(tab + o.kc), tab + o.rows);

		// every trace of the round once: a forward call per stretch of contiguous traces
		for (size_t j = r.j0; j < r.j1;) {
			size_t k = j + 1, nt = E[j].m;
			while (k < r.j1 && E[k].f == E[k - 1].f + E[k - 1].m) nt += E[k++].m;
			if ((rc = tspws_forward_parts<float>(pl, d_x + E[j].f * ld, nt, ld, part + (size_t)he[j - r.j0].part0 * pl->npart, st, nullptr, ScaleRange()))) return rc;
			j = k;
		}
		for (unsigned g0 = 0; g0 < ng; g0 += 65535)
			hipLaunchKernelGGL(k_rb_accumulate<P>, dim3(pl->acc_blocks, std::min(65535u, ng - g0), (unsigned)ne), dim3(256), 0, st, (const double2 *)part, pl->npart,
			                   (const ScaleDesc *)pl->d_sc, pl->S, nc, d_ens, d_codes, M, g0, planes);
		for (unsigned q0 = 0; q0 < M; q0 += 65535)
			hipLaunchKernelGGL(k_rb_linear<P>, dim3(nb256, std::min(65535u, M - q0), (unsigned)ne), dim3(256), 0, st, d_x, ld, N, d_ens, d_codes, d_rows, M, q0, d_ls_out);
		// finish: the rows of the round in even batches
		for (size_t r0 = 0; r0 < nrows; r0 += RB) {
			const unsigned nr = (unsigned)std::min(RB, nrows - r0);
			P::launch_weight(dim3((unsigned)((nc + 255) / 256), nr), st, OUT, (const double2 *)planes, nc, d_rows, r0, p);
			if ((rc = tspws_hip_inverse(pl, (const double *)OUT, nr, xr, (void *)st))) return rc;
			hipLaunchKernelGGL(k_sb_epilogue, dim3(nb256, nr), dim3(256), 0, st, (const double *)xr, N, d_ens, d_rows.kc, M, r0, d_ts_out);
		}
		round_end(d_ens, d_rows.kc, (unsigned)ne);
	}
	return 0;
}

// what the entries refuse, in the order of the other batch calls: first what needs no plan, then the caller's own checks that need none
// (own(): 0 or its refusal), then the plan's.  two_stage: NULL where two-stage ensembles (0 < Kmax <= traces) are taken -- then within
// M + 2 <= 65535 and M Kmax < 2^32 --, else the sentence that refuses one.  *done: nothing to do (B == 0 or M == 0)
template <class Own>
static int row_batch_check(const char *call, const char *two_stage, const tspws_hip_plan *pl, const t_tsPWS *p, const float *d_x, size_t ld, const size_t *h_first, unsigned B,
                           unsigned M, bool matrix_ok, const float *d_ls_out, const float *d_ts_out, const unsigned *h_mtr_out, bool *done, Own own)
{
	const std::string name = call;
	auto refuse = [&](const std::string &what) { return fail(TSPWS_E_ARG, (name + ": " + what).c_str()); };
	*done = false;
	if (!p || !h_first) return refuse("NULL");
	if (!B || !M) { *done = true; return pl ? 0 : refuse("NULL"); }
	if (!matrix_ok || !d_ls_out || !d_ts_out || !h_mtr_out) return refuse("NULL");
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] < h_first[b]) return refuse("decreasing ensemble offsets");
	bool two = false;
	for (unsigned b = 0; b < B; b++) {
		const size_t m = h_first[b + 1] - h_first[b];
		if (m > 0xfffffff0ull) return refuse("more than 2^32 traces in an ensemble");
		two |= m && tspws_is_two_stage(p, m);
		if (two && two_stage) return refuse(two_stage);
	}
	if (two && ((size_t)M + 2 > 65535 || (size_t)M * p->Kmax > 0xffffffffull)) return refuse("too many masks for two-stage ensembles (M + 2 <= 65535, M Kmax < 2^32)");
	if (int rc = own()) return rc;
	if (!pl) return refuse("NULL");
	const size_t Tn = h_first[B] - h_first[0];
	if (Tn && !d_x) return refuse("NULL traces");
	if (Tn && ld < pl->N) return refuse("row stride below the trace length");
	return 0;
}
