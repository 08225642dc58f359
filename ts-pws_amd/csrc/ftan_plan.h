// ftan_plan.h -- how the group-arrival calls (ftan_rows.hip: tspws_hip_ftan_coef, tspws_hip_ftan_rows) cut their work: the classes of
// ensembles, per class the work items that all rows of its ensembles share, the tasks a wave takes, the rounds, and the ONE table block a
// pass uploads.  Host code only, no HIP runtime: tests/ftan_plan_check.cpp compiles it with a plain C++17 compiler.
//
// CLASSES.  Every ensemble has its own W windows (station pairs differ in distance) and, when noise is wanted, its own noise range.
// Ensembles whose window sets and noise ranges are equal by value share one class, numbered in order of first appearance.
// RANGES.  The members of (scale, window) are the indices wx_k_range (wxs_plan.h) gives: ceil(n0 / D) <= k < ceil(n1 / D), and under the wrap
// rule the filter support inside [0, N).  The noise range [q0, q1) likewise.
// ITEMS.  Per class, the members of (scale, window) are cut into segments of FT_SEG counted from the FIRST member, and so are the members of
// (scale, noise range): the segments depend on that scale, that range and the wrap rule alone.  Items are listed by class; inside a class
// the peak items by (scale, window, segment), then the noise items by (scale, segment).  pspans[(class Sx + sx) W + w] and
// nspans[class Sx + sx] bracket them.  An empty range has no item.  An item carries its scale's offset and length: the neighbours of a
// member are indices of the SCALE, so the kernel reads one coefficient on either side of the segment.
// TASKS.  A wave takes a run of consecutive items of ONE class of at most FT_TASK passes of 64 coefficients, one after the other, each with
// its own result (WX_TASK's principle).  A pass runs max_tasks waves per participating row; a row of a class with fewer tasks ends the rest.
// ROUNDS.  tspws_hip_ftan_rows: whole ensembles whose M coefficient sets, partial results and table stay inside the parts budget; the first
// ensemble of a round is always taken.  tspws_hip_ftan_coef (the sets are the caller's): chunks of rows whose partial results and table do.
// The round rule, the slots, the chunk search and the task packing are host_plan.h's.
#pragma once

#include "wxs_plan.h" // WxScale, wx_k_range; host_plan.h

#include <map>

enum { FT_SEG = 256, FT_TASK = 16, FT_WMAX = 4, FT_PMAX = 4 };

// members [k0, k0 + count) of a scale of Ns coefficients that starts at `base` of a row's set; noise != 0: an item of the noise range
struct FtItem { unsigned long long base; unsigned k0, count, Ns, noise; };
struct FtTask { unsigned first, n; };                       // items [first, first + n), of one class
struct FtSpan { unsigned first, n; };                       // items of (class, scale, window) or (class, scale)
struct FtClass { unsigned item0, nitems, task0, ntasks; };  // the class's items and tasks
struct FtScale { unsigned long long base; unsigned D, Ns; }; // scale s_begin + sx
struct FtRow { unsigned row, cls; };                        // a participating row and its ensemble's class

struct FtPlan {
	unsigned W = 0, Sx = 0, max_items = 0, max_tasks = 0;
	bool noise = false;
	std::vector<unsigned> cls_of;   // [B]: class of every ensemble
	std::vector<unsigned> first_of; // [classes]: the first ensemble of the class
	std::vector<FtItem> items;
	std::vector<FtTask> tasks;
	std::vector<FtClass> classes;
	std::vector<FtSpan> pspans;     // [classes][Sx][W]
	std::vector<FtSpan> nspans;     // [classes][Sx] (noise wanted)
	std::vector<FtScale> scales;    // [Sx]
};

// win: [B][W] pairs n0 < n1 <= N, 1 <= W <= FT_WMAX; noise: NULL or [B] pairs q0 < q1 <= N; scales [s_begin, s_end), s_begin < s_end <= S
inline FtPlan ft_plan(const WxScale *sc, unsigned S, size_t N, unsigned s_begin, unsigned s_end, const size_t *win, unsigned W, const size_t *noise, size_t B,
                      int skip_wrapped)
{
	(void)S;
	FtPlan p;
	p.W = W; p.Sx = s_end - s_begin; p.noise = noise != nullptr;
	for (unsigned s = s_begin; s < s_end; s++) p.scales.push_back({sc[s].coef_off, sc[s].D, sc[s].Ns});
	std::map<std::vector<size_t>, unsigned> id;
	p.cls_of.resize(B);
	for (size_t b = 0; b < B; b++) {
		std::vector<size_t> key(win + b * W * 2, win + (b + 1) * W * 2);
		if (noise) key.insert(key.end(), noise + 2 * b, noise + 2 * b + 2);
		auto it = id.find(key);
		if (it == id.end()) { it = id.emplace(key, (unsigned)p.first_of.size()).first; p.first_of.push_back((unsigned)b); }
		p.cls_of[b] = it->second;
	}
	auto cut = [&](const WxScale &s, size_t n0, size_t n1, unsigned kind) {
		size_t k0, k1;
		wx_k_range(s, N, n0, n1, skip_wrapped, &k0, &k1);
		FtSpan sp = {(unsigned)p.items.size(), 0};
		for (size_t k = k0; k < k1; k += FT_SEG, sp.n++) p.items.push_back({s.coef_off, (unsigned)k, (unsigned)std::min<size_t>(FT_SEG, k1 - k), s.Ns, kind});
		return sp;
	};
	for (unsigned c = 0; c < p.first_of.size(); c++) {
		const size_t b = p.first_of[c];
		FtClass cl = {(unsigned)p.items.size(), 0, (unsigned)p.tasks.size(), 0};
		for (unsigned s = s_begin; s < s_end; s++)
			for (unsigned w = 0; w < W; w++) p.pspans.push_back(cut(sc[s], win[(b * W + w) * 2], win[(b * W + w) * 2 + 1], 0));
		if (noise)
			for (unsigned s = s_begin; s < s_end; s++) p.nspans.push_back(cut(sc[s], noise[2 * b], noise[2 * b + 1], 1));
		cl.nitems = (unsigned)p.items.size() - cl.item0;
		pack_tasks(p.tasks, cl.item0, cl.item0 + cl.nitems, FT_TASK, [&](unsigned i) { return (p.items[i].count + 63) / 64; },
		           [&](unsigned i) { return i == cl.item0; }); // (no task crosses a class)
		cl.ntasks = (unsigned)p.tasks.size() - cl.task0;
		p.classes.push_back(cl);
		p.max_items = std::max(p.max_items, cl.nitems);
		p.max_tasks = std::max(p.max_tasks, cl.ntasks);
	}
	return p;
}

// the table block of a pass over nrows rows of which nslots take part:
// items | tasks | classes | peak spans | noise spans | scales | the participating rows | slot of every row or NOSLOT
struct FtTab { size_t items, tasks, classes, pspans, nspans, scales, list, slot_of, bytes; };
inline FtTab ft_tab(const FtPlan &p, size_t nslots, size_t nrows)
{
	TableLayout lay;
	FtTab t;
	t.items = lay.add<FtItem>(p.items.size()); t.tasks = lay.add<FtTask>(p.tasks.size()); t.classes = lay.add<FtClass>(p.classes.size());
	t.pspans = lay.add<FtSpan>(p.pspans.size()); t.nspans = lay.add<FtSpan>(p.nspans.size()); t.scales = lay.add<FtScale>(p.scales.size());
	t.list = lay.add<FtRow>(nslots); t.slot_of = lay.add<unsigned>(nrows);
	t.bytes = lay.bytes;
	return t;
}

// the partial results of a pass: [slot][max_items][P] entries of 16 bytes ((a2, k) of a peak item's r-th peak; (Q, n) in entry 0 of a noise item)
inline size_t ft_part_bytes(const FtPlan &p, unsigned P, size_t nslots) { return nslots * p.max_items * P * 16; }
// what a pass over nrows rows holds beside the coefficient sets, at most (every row taking part)
inline size_t ft_pass_bytes(const FtPlan &p, unsigned P, size_t nrows) { return ft_part_bytes(p, P, nrows) + ft_tab(p, nrows, nrows).bytes; }
// the coefficient sets of nb ensembles of M rows
inline size_t ft_set_bytes(size_t nb, size_t M, size_t ncoef) { return nb * M * ncoef * 2 * sizeof(double); }

// tspws_hip_ftan_rows: rounds of whole ensembles
inline std::vector<Round> ft_rounds(size_t B, size_t M, size_t ncoef, const FtPlan &p, unsigned P, size_t budget)
{
	return whole_ensemble_rounds(B, [&](size_t j0, size_t j1) {
		const size_t a = ft_set_bytes(j1 - j0, M, ncoef), b = ft_pass_bytes(p, P, (j1 - j0) * M);
		return a <= budget && b <= budget - a;
	});
}

// tspws_hip_ftan_coef: the rows of a chunk (at least one; ft_pass_bytes is monotone in the rows)
inline size_t ft_chunk_rows(size_t nrow, const FtPlan &p, unsigned P, size_t budget)
{
	return largest_fitting(nrow, [&](size_t n) { return ft_pass_bytes(p, P, n); }, budget);
}

// the table of a pass into blob (ft_tab's layout for the pass's own counts; zeroed by the caller); ens[nrows] = the ensemble (of the call's B)
// of every row, or NOSLOT for a row that does not take part.  Returns the participating rows.
inline size_t ft_fill(char *blob, const FtTab &t, const FtPlan &p, const unsigned *ens, size_t nrows)
{
	std::copy(p.items.begin(), p.items.end(), (FtItem *)(blob + t.items));
	std::copy(p.tasks.begin(), p.tasks.end(), (FtTask *)(blob + t.tasks));
	std::copy(p.classes.begin(), p.classes.end(), (FtClass *)(blob + t.classes));
	std::copy(p.pspans.begin(), p.pspans.end(), (FtSpan *)(blob + t.pspans));
	std::copy(p.nspans.begin(), p.nspans.end(), (FtSpan *)(blob + t.nspans));
	std::copy(p.scales.begin(), p.scales.end(), (FtScale *)(blob + t.scales));
	FtRow *list = (FtRow *)(blob + t.list);
	return fill_row_slots((unsigned *)(blob + t.slot_of), ens, nrows, [&](size_t slot, unsigned e, size_t i) { list[slot] = {(unsigned)i, p.cls_of[e]}; });
}
