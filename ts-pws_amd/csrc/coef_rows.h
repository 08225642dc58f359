// coef_rows.h -- the two drivers that the units working on coefficient sets share (wxs_rows.hip, ftan_rows.hip): rows whose sets are the
// caller's, in chunks (*_coef), and stack rows [B][M][ld] transformed round by round with tspws_hip_forward_f32 (*_rows).  A driver owns the ens
// vector, the counters of the call's stats, the sizes every pass reserves and the call's end; the unit's pass builds its table and launches its
// kernels:  pass(Y, Yref, ens, n, row0, max_rows) -> rc  takes the sets Y of n rows (Yref: the reference sets, where the unit has any),
// ens[i] = the ensemble of row i or NOSLOT, writes the outputs from row `row0` on and reserves its slots for the largest pass's max_rows rows,
// so that no slot grows between passes.
#pragma once

#include "batch_host.h"
#include "wxs_plan.h"

struct RowCounters { unsigned &rounds, &rows, &left_out; }; // (what the stats of both units count alike)
template <class Stats>
static inline RowCounters row_counters(Stats &s) { return {s.rounds, s.rows, s.left_out}; }

// what the plans need of the frame's scales (omega: the caller's)
static inline std::vector<WxScale> wx_scales_of(const tspws_hip_plan *pl)
{
	std::vector<WxScale> sc(pl->S);
	for (unsigned s = 0; s < pl->S; s++) {
		const ScaleDesc &d = pl->sc[s];
		sc[s] = {d.L, d.D, d.Ns, d.c, d.coef_off, 0.0};
	}
	return sc;
}

// the rows [0, nrow) of Y in chunks of `chunk`; h_ens[i] = the ensemble of row i (NULL: i).  Every row takes part.
template <class Pass>
static int coef_chunks(BatchCall &call, RowCounters n, const double2 *Y, const double2 *Yref, size_t ncoef, const unsigned *h_ens, size_t nrow, size_t chunk, Pass pass)
{
	n.rows = (unsigned)nrow;
	std::vector<unsigned> ens(chunk);
	for (size_t r0 = 0; r0 < nrow; r0 += chunk) {
		const size_t k = std::min(chunk, nrow - r0);
		for (size_t i = 0; i < k; i++) ens[i] = h_ens ? h_ens[r0 + i] : (unsigned)(r0 + i);
		n.rounds++;
		if (int rc = pass(Y + r0 * ncoef, Yref, (const unsigned *)ens.data(), k, r0, chunk)) return rc;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}

// the stack rows round by round: the sets of the round's nb M rows, then of its nb nref references (d_ref[B][ldr]; nref = 0: none), in the
// scratch slot `slot`.  With references a row's ens is its ensemble's index in the round, which is its reference's set; without, the ensemble
// of the call.
template <class Pass>
static int coef_rounds(tspws_hip_plan *pl, BatchCall &call, RowCounters n, const float *d_rows, size_t ld, unsigned M, const unsigned *h_mtr, const float *d_ref,
                       size_t ldr, unsigned nref, const std::vector<Round> &rounds, int slot, Pass pass)
{
	hipStream_t st = call.stream();
	const size_t ncoef = pl->ncoef;
	size_t max_nb = 0;
	for (const Round &r : rounds) max_nb = std::max(max_nb, r.j1 - r.j0);
	int rc;
	void *v;
	if ((rc = scratch(pl, slot, std::max<size_t>(max_nb * (M + nref) * ncoef * sizeof(double2), 16), &v))) return rc; // (the largest round's)
	double2 *Y = (double2 *)v;
	std::vector<unsigned> ens(max_nb * M);
	for (const Round &r : rounds) {
		const size_t nb = r.j1 - r.j0, nrows = nb * M;
		double2 *Yref = Y + nrows * ncoef;
		// the rows left out are transformed too: ONE forward call on the round's rows, one on its references
		if ((rc = tspws_hip_forward_f32(pl, d_rows + r.j0 * M * ld, nrows, ld, (double *)Y, st))) return rc;
		if (nref && (rc = tspws_hip_forward_f32(pl, d_ref + r.j0 * ldr, nb, ldr, (double *)Yref, st))) return rc;
		for (size_t bl = 0; bl < nb; bl++)
			for (size_t m = 0; m < M; m++) {
				const bool in = !h_mtr || h_mtr[(r.j0 + bl) * M + m] > 0;
				ens[bl * M + m] = in ? (unsigned)(nref ? bl : r.j0 + bl) : NOSLOT;
				n.rows += in;
				n.left_out += !in;
			}
		n.rounds++;
		if ((rc = pass((const double2 *)Y, (const double2 *)Yref, (const unsigned *)ens.data(), nrows, r.j0 * M, max_nb * M))) return rc;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(call.drain()); // outputs complete
	return 0;
}
