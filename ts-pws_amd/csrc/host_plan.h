// host_plan.h -- what the host plans share: the layout of a table block, the rounds of whole ensembles, which rows take part and the slot each
// gets, the largest count within a budget, the packing of items into tasks and the check of a range list.  The ONE statement of each rule for
// the batched calls (batch_host.h), the run tables (column_runs.h) and the five row-analysis plans (stretch_plan.h, wxs_plan.h, mwcs_plan.h,
// dtw_plan.h, ftan_plan.h).  Host code only, no HIP runtime: tests/host_plan_check.cpp compiles it with a plain C++17 compiler.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

// The layout of a table block: the arrays one after the other, each aligned for its element type.  A unit states its block ONCE, as a function of
// the arrays' lengths; with upper bounds of the lengths the same function gives an upper bound of the block (add is monotone in count, whatever
// came before), which is what plans the rounds of the batched calls.
struct TableLayout {
	size_t bytes = 0;
	template <class T>
	size_t add(size_t count) // offset of an array of `count` T
	{
		const size_t o = (bytes + alignof(T) - 1) / alignof(T) * alignof(T);
		bytes = o + count * sizeof(T);
		return o;
	}
};

// Rounds of whole ensembles [j0, j1) of a list of n: the first ensemble of a round is always taken (one alone may exceed the budget), the
// round extends while fits(j0, j1 + 1) says that the ensembles [j0, j1 + 1) fit together.
struct Round { size_t j0, j1; };
template <class Fits>
static inline std::vector<Round> whole_ensemble_rounds(size_t n, Fits fits)
{
	std::vector<Round> rounds;
	for (size_t j0 = 0, j1; j0 < n; j0 = j1) {
		j1 = j0 + 1;
		while (j1 < n && fits(j0, j1 + 1)) j1++;
		rounds.push_back({j0, j1});
	}
	return rounds;
}

// PARTICIPATION.  Row (b, m) of the stack rows [B][M] takes part iff h_mtr == NULL or h_mtr[b M + m] > 0.  The rows of a pass that take part
// get the SLOTS 0, 1, .. in row order; the others get NOSLOT.
constexpr unsigned NOSLOT = ~0u;

// nrows0[b] = participating rows in front of ensemble b (B + 1 entries)
inline std::vector<size_t> participating_rows0(const unsigned *h_mtr, size_t B, size_t M)
{
	std::vector<size_t> nrows0(B + 1, 0);
	for (size_t b = 0; b < B; b++) {
		size_t n = M;
		if (h_mtr) { n = 0; for (size_t m = 0; m < M; m++) n += h_mtr[b * M + m] > 0; }
		nrows0[b + 1] = nrows0[b] + n;
	}
	return nrows0;
}

// slot_of[(b - r.j0) M + m] of the ensembles of round r from h_mtr; each(slot, b, m) for every participating row in order.  Returns their number.
template <class Each>
inline size_t fill_round_slots(unsigned *slot_of, const Round &r, size_t M, const unsigned *h_mtr, Each each)
{
	size_t slot = 0;
	for (size_t b = r.j0; b < r.j1; b++)
		for (size_t m = 0; m < M; m++) {
			const bool in = !h_mtr || h_mtr[b * M + m] > 0;
			slot_of[(b - r.j0) * M + m] = in ? (unsigned)slot : NOSLOT;
			if (in) each(slot++, b, m);
		}
	return slot;
}

// slot_of[i] of the rows [0, nrows) from ens[i] = the row's ensemble, or NOSLOT for a row that does not take part; each(slot, ens[i], i)
template <class Each>
inline size_t fill_row_slots(unsigned *slot_of, const unsigned *ens, size_t nrows, Each each)
{
	size_t slot = 0;
	for (size_t i = 0; i < nrows; i++) {
		slot_of[i] = ens[i] == NOSLOT ? NOSLOT : (unsigned)slot;
		if (ens[i] != NOSLOT) each(slot++, ens[i], i);
	}
	return slot;
}

inline size_t count_slots(const unsigned *ens, size_t nrows)
{
	size_t n = 0;
	for (size_t i = 0; i < nrows; i++) n += ens[i] != NOSLOT;
	return n;
}

// the largest k in [1, n] with bytes_of(k) <= budget (bytes_of is monotone in k); 1 when none fits
template <class BytesOf>
inline size_t largest_fitting(size_t n, BytesOf bytes_of, size_t budget)
{
	size_t lo = 1, hi = n;
	while (lo < hi) {
		const size_t mid = lo + (hi - lo + 1) / 2;
		if (bytes_of(mid) <= budget) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// TASKS.  The items [i0, i1) in runs of consecutive items {first, n} behind `tasks`: a run holds at most `limit` passes (item i is passes_of(i)
// passes; one item alone always fits) and extends as far as that allows, but a new run starts at every item with restart(i) (and at the first
// item when `tasks` is empty).
template <class Task, class PassesOf, class Restart>
inline void pack_tasks(std::vector<Task> &tasks, unsigned i0, unsigned i1, unsigned limit, PassesOf passes_of, Restart restart)
{
	unsigned passes = 0;
	for (unsigned i = i0; i < i1; i++) {
		const unsigned c = passes_of(i);
		if (tasks.empty() || restart(i) || passes + c > limit) { tasks.push_back({i, 0}); passes = 0; }
		tasks.back().n++;
		passes += c;
	}
}

// RANGES.  A call takes 1 to RANGE_MAX ranges [n0, n1), n0 < n1 <= N, as pairs win[2 w], win[2 w + 1]; the calls name them windows or lag
// ranges.  Each check returns what is wrong (the tail of the message, the caller prefixes its name) or NULL; an entry point makes them in
// its own order.
enum { RANGE_MAX = 4 };
struct RangeWords { const char *count, *empty, *past; };
constexpr RangeWords WINDOWS = {"1 to 4 windows", "an empty window (n0 >= n1)", "a window past the trace length"};
constexpr RangeWords LAG_RANGES = {"1 to 4 lag ranges", "an empty lag range (n0 >= n1)", "a lag range past the trace length"};

inline const char *range_count_error(unsigned W, const RangeWords &what) { return !W || W > RANGE_MAX ? what.count : nullptr; }
inline const char *range_empty_error(const size_t *win, size_t count, const RangeWords &what) // (count: all ranges of the list, W per ensemble)
{
	for (size_t w = 0; w < count; w++)
		if (win[2 * w] >= win[2 * w + 1]) return what.empty;
	return nullptr;
}
// what needs no plan: the count, then the empty ranges
inline const char *range_error(const size_t *win, unsigned W, const RangeWords &what)
{
	const char *e = range_count_error(W, what);
	return e ? e : range_empty_error(win, W, what);
}
// the second call, once the plan is known
inline const char *range_past_error(const size_t *win, size_t count, size_t N, const RangeWords &what)
{
	for (size_t w = 0; w < count; w++)
		if (win[2 * w + 1] > N) return what.past;
	return nullptr;
}
