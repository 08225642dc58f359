// filter_plan.h -- the host plan of the coherence filter (filter_traces.hip): what a target row and an ensemble cost, the rounds of whole
// ensembles, the chunks of an ensemble that exceeds the budget alone, the slabs of a pass and its table block.  Host code only, no HIP
// runtime: tests/filter_plan_check.cpp compiles it with a plain C++17 compiler.  The rounds, the largest fit, participation and the table
// layout are host_plan.h's.
//
// A PASS is a run of consecutive target rows whose coefficient sets lie side by side; ens[i] names the ensemble of row i among the pass's
// ensembles, NOSLOT a row that is left out.  A SLAB is up to CF_SLAB consecutive participating rows of one ensemble: the unit of work of
// k_cf_apply.  A row that is left out belongs to no slab and ends the one in front of it.
#pragma once

#include "host_plan.h"

constexpr unsigned CF_SLAB = 8;
constexpr size_t CF_MAX_ENS = 65535; // ensembles of a pass (grid.y of k_cf_weight)

struct CfSlab { unsigned row0, n, ens; };      // rows [row0, row0 + n) of the pass, 1 <= n <= CF_SLAB, of the pass's ensemble `ens`
struct CfEns { double K; int mode; unsigned pad; }; // the count and the weight's mode in force for the ensemble (leave-one-out: K - 1 and its mode)

inline std::vector<CfSlab> cf_slabs(const unsigned *ens, size_t nrows)
{
	std::vector<CfSlab> slabs;
	for (size_t i = 0; i < nrows; i++) {
		if (ens[i] == NOSLOT) continue;
		const bool fresh = slabs.empty() || slabs.back().ens != ens[i] || slabs.back().n == CF_SLAB || (size_t)slabs.back().row0 + slabs.back().n != i;
		if (fresh) slabs.push_back({(unsigned)i, 0u, ens[i]});
		slabs.back().n++;
	}
	return slabs;
}

// What stays within the budget.  Per target row: its coefficient set and its FP64 row of the inverse.  Per ensemble: its PS plane and its W
// plane.  Once per pass (fixed): the ST plane that the accumulation writes beside PS and the partial-stack rows of a two-stage ensemble.
// (The transforms' own scratch -- the forward's partials, the inverse's octave buffer -- is theirs to keep within the same budget: the forward
// batches its traces itself, the inverse is called on cf_inverse_rows rows at a time.)
struct CfCost { size_t row_bytes, ens_bytes, fixed; };
inline CfCost cf_cost(size_t ncoef, size_t N, unsigned Kmax)
{
	return {ncoef * 16 + N * 8, ncoef * (16 + 8), ncoef * 16 + (size_t)Kmax * N * 8};
}
// rows of one tspws_hip_inverse call: even (the inverse pairs its rows), at inv_row_bytes a row (tspws_inverse_row_bytes) within the budget
inline size_t cf_inverse_rows(size_t nrows, size_t inv_row_bytes, size_t budget)
{
	return std::min(nrows, std::max<size_t>(2, (budget / inv_row_bytes) & ~(size_t)1));
}
inline size_t cf_bytes(const CfCost &c, size_t nens, size_t nrows) { return c.fixed + nens * c.ens_bytes + nrows * c.row_bytes; }

// rounds of whole ensembles; rows0[b] = target rows in front of ensemble b (B + 1 entries).  One ensemble alone may exceed the budget:
// cf_round_fits tells, and such a round is worked in chunks of cf_chunk_rows rows
inline std::vector<Round> cf_rounds(const size_t *rows0, size_t B, const CfCost &c, size_t budget)
{
	return whole_ensemble_rounds(B, [&](size_t j0, size_t j1) { return j1 - j0 <= CF_MAX_ENS && cf_bytes(c, j1 - j0, rows0[j1] - rows0[j0]) <= budget; });
}
inline bool cf_round_fits(const size_t *rows0, const Round &r, const CfCost &c, size_t budget)
{
	return cf_bytes(c, r.j1 - r.j0, rows0[r.j1] - rows0[r.j0]) <= budget;
}
inline size_t cf_chunk_rows(size_t nrows, const CfCost &c, size_t budget)
{
	return largest_fitting(nrows, [&](size_t k) { return cf_bytes(c, 1, k); }, budget);
}

// the table block of a pass: the slabs, the ensembles' counts and modes, and per row whether it takes part (k_cf_rows)
struct CfTab { size_t slabs, ens, live, bytes; };
inline CfTab cf_tab(size_t nslabs, size_t nens, size_t nrows)
{
	TableLayout lay;
	CfTab o;
	o.ens = lay.add<CfEns>(nens);
	o.slabs = lay.add<CfSlab>(nslabs);
	o.live = lay.add<unsigned>(nrows);
	o.bytes = lay.bytes;
	return o;
}
inline void cf_fill(char *blob, const CfTab &o, const std::vector<CfSlab> &slabs, const CfEns *en, size_t nens, const unsigned *ens, size_t nrows)
{
	std::copy(en, en + nens, (CfEns *)(blob + o.ens));
	std::copy(slabs.begin(), slabs.end(), (CfSlab *)(blob + o.slabs));
	unsigned *live = (unsigned *)(blob + o.live);
	for (size_t i = 0; i < nrows; i++) live[i] = ens[i] != NOSLOT;
}
