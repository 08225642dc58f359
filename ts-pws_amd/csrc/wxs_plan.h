// wxs_plan.h -- how the wavelet cross-spectrum calls (wxs_rows.hip: tspws_hip_wxs_coef, tspws_hip_wxs_rows) cut their work: the scales in use,
// per (scale, window) the range of coefficient indices after the wrap rule, the work items that all rows share, the tasks a wave takes, the
// rounds, and the ONE table block a pass uploads.  Host code only, no HIP runtime: tests/wxs_plan_check.cpp compiles it with a plain C++17
// compiler.
//
// SCALES IN USE.  A scale inside at least one band of the table, in increasing s.  Only these are read.
// RANGES.  Coefficient k of scale s sits at sample k D_s.  It lies in window [n0, n1) iff ceil(n0 / D) <= k < ceil(n1 / D); with the wrap rule
// its filter support [k D - c, k D - c + L) must also lie inside [0, N): ceil(c / D) <= k (c > 0) and k D <= N + c - L.
// ITEMS.  The range of (scale in use, window) is cut into segments of WX_SEG coefficients counted from ITS first index, so the segments -- and
// with them the order of every sum -- depend on that scale, that window and the wrap rule alone, not on the band table or the other windows.
// Items are listed by (scale in use, window, segment); spans[u W + w] brackets the items of (u, w).  An empty range has no item.
// TASKS.  A wave takes a run of consecutive items of at most WX_TASK passes of 64 coefficients (an item is ceil(count / 64) passes; one item
// alone always fits: WX_SEG = 4 passes), one after the other, each with its own sums and its own reduction: the coarse scales' many short
// items share waves, and no item's sum depends on the run it is in.
// ROUNDS.  tspws_hip_wxs_rows: whole ensembles whose coefficient sets ((M + 1) sets of ncoef complex doubles each), partial sums and table
// stay inside the parts budget; the first ensemble of a round is always taken.  tspws_hip_wxs_coef (the sets are the caller's): chunks of
// rows whose partial sums and table do.  The round rule, the slots, the chunk search and the task packing are host_plan.h's.
#pragma once

#include "host_plan.h"

#include <cstdint>

enum { WX_SEG = 256, WX_TASK = 16, WX_WMAX = 4, WX_RMAX = 64, WX_NSUM = 9, WX_NFIT = 6 };

struct WxScale { unsigned L, D, Ns; int c; unsigned long long coef_off; double omega; }; // what the plan needs of a scale (omega = w0 / scale)
struct WxBand { unsigned s_begin, s_end; };                                              // (tspws_band)
// coefficients [coef, coef + count) of a row's set: the indices k0 .. of its scale, which sit at the samples (k0 + j) D
struct WxItem { unsigned long long coef; unsigned k0, count, D, pad; double omega; };
struct WxTask { unsigned first, n; }; // items [first, first + n)
struct WxSpan { unsigned first, n; }; // items of (scale in use, window)
struct WxRow { unsigned row, ens; };  // a participating row: its coefficient set in Yc, its reference's in Yr

struct WxPlan {
	unsigned W = 0;
	std::vector<unsigned> used;  // scales in use, increasing
	std::vector<unsigned> uidx;  // [S]: index into used, or NOSLOT
	std::vector<WxItem> items;
	std::vector<WxTask> tasks;
	std::vector<WxSpan> spans;   // [used][W]
};

// the indices [*k0, *k1) of scale sc inside window [n0, n1), n0 < n1 <= N (*k0 == *k1: none)
inline void wx_k_range(const WxScale &sc, size_t N, size_t n0, size_t n1, int skip_wrapped, size_t *k0, size_t *k1)
{
	const long long D = sc.D;
	long long a = ((long long)n0 + D - 1) / D, b = std::min<long long>(((long long)n1 + D - 1) / D, sc.Ns);
	if (skip_wrapped) {
		if (sc.c > 0) a = std::max(a, ((long long)sc.c + D - 1) / D);
		const long long last = (long long)N + sc.c - (long long)sc.L; // the largest k D whose support ends inside the trace
		b = last < 0 ? a : std::min(b, last / D + 1);
	}
	if (b < a) b = a;
	*k0 = (size_t)a; *k1 = (size_t)b;
}

// bands: R ranges inside [0, S] (checked by the caller); win: W pairs n0 < n1 <= N, 1 <= W <= WX_WMAX
inline WxPlan wx_plan(const WxScale *sc, unsigned S, size_t N, const WxBand *bands, unsigned R, const size_t *win, unsigned W, int skip_wrapped)
{
	WxPlan p;
	p.W = W;
	p.uidx.assign(S, NOSLOT);
	std::vector<char> in(S, 0);
	for (unsigned r = 0; r < R; r++)
		for (unsigned s = bands[r].s_begin; s < bands[r].s_end; s++) in[s] = 1;
	for (unsigned s = 0; s < S; s++)
		if (in[s]) { p.uidx[s] = (unsigned)p.used.size(); p.used.push_back(s); }
	for (unsigned s : p.used)
		for (unsigned w = 0; w < W; w++) {
			size_t k0, k1;
			wx_k_range(sc[s], N, win[2 * w], win[2 * w + 1], skip_wrapped, &k0, &k1);
			WxSpan sp = {(unsigned)p.items.size(), 0};
			for (size_t k = k0; k < k1; k += WX_SEG, sp.n++) {
				WxItem it;
				it.coef = sc[s].coef_off + k; it.k0 = (unsigned)k; it.count = (unsigned)std::min<size_t>(WX_SEG, k1 - k); it.D = sc[s].D; it.pad = 0;
				it.omega = sc[s].omega;
				p.items.push_back(it);
			}
			p.spans.push_back(sp);
		}
	pack_tasks(p.tasks, 0, (unsigned)p.items.size(), WX_TASK, [&](unsigned i) { return (p.items[i].count + 63) / 64; }, [](unsigned) { return false; });
	return p;
}

// the table block of a pass over nrows rows of which nslots take part:
// items | tasks | spans | index of every scale in `used` | bands | the participating rows | slot of every row or NOSLOT
struct WxTab { size_t items, tasks, spans, uidx, bands, list, slot_of, bytes; };
inline WxTab wx_tab(const WxPlan &p, unsigned R, size_t nslots, size_t nrows)
{
	TableLayout lay;
	WxTab t;
	t.items = lay.add<WxItem>(p.items.size()); t.tasks = lay.add<WxTask>(p.tasks.size()); t.spans = lay.add<WxSpan>(p.spans.size());
	t.uidx = lay.add<unsigned>(p.uidx.size()); t.bands = lay.add<WxBand>(R); t.list = lay.add<WxRow>(nslots); t.slot_of = lay.add<unsigned>(nrows);
	t.bytes = lay.bytes;
	return t;
}

// the partial sums of a pass: [slot][item][WX_NSUM] doubles
inline size_t wx_part_bytes(const WxPlan &p, size_t nslots) { return nslots * p.items.size() * WX_NSUM * sizeof(double); }
// what a pass over nrows rows holds beside the coefficient sets, at most (every row taking part)
inline size_t wx_pass_bytes(const WxPlan &p, unsigned R, size_t nrows) { return wx_part_bytes(p, nrows) + wx_tab(p, R, nrows, nrows).bytes; }
// the coefficient sets of nb ensembles of M rows and one reference
inline size_t wx_set_bytes(size_t nb, size_t M, size_t ncoef) { return nb * (M + 1) * ncoef * 2 * sizeof(double); }

// tspws_hip_wxs_rows: rounds of whole ensembles
inline std::vector<Round> wx_rounds(size_t B, size_t M, size_t ncoef, const WxPlan &p, unsigned R, size_t budget)
{
	return whole_ensemble_rounds(B, [&](size_t j0, size_t j1) {
		const size_t a = wx_set_bytes(j1 - j0, M, ncoef), b = wx_pass_bytes(p, R, (j1 - j0) * M);
		return a <= budget && b <= budget - a;
	});
}

// tspws_hip_wxs_coef: the rows of a chunk (at least one; wx_pass_bytes is monotone in the rows)
inline size_t wx_chunk_rows(size_t nrow, const WxPlan &p, unsigned R, size_t budget)
{
	return largest_fitting(nrow, [&](size_t n) { return wx_pass_bytes(p, R, n); }, budget);
}

// the table of a pass into blob (wx_tab's layout for the pass's own counts; zeroed by the caller); ens[nrows] = the reference set of every
// row, or NOSLOT for a row that does not take part.  Returns the participating rows.
inline size_t wx_fill(char *blob, const WxTab &t, const WxPlan &p, const WxBand *bands, unsigned R, const unsigned *ens, size_t nrows)
{
	std::copy(p.items.begin(), p.items.end(), (WxItem *)(blob + t.items));
	std::copy(p.tasks.begin(), p.tasks.end(), (WxTask *)(blob + t.tasks));
	std::copy(p.spans.begin(), p.spans.end(), (WxSpan *)(blob + t.spans));
	std::copy(p.uidx.begin(), p.uidx.end(), (unsigned *)(blob + t.uidx));
	std::copy(bands, bands + R, (WxBand *)(blob + t.bands));
	WxRow *list = (WxRow *)(blob + t.list);
	return fill_row_slots((unsigned *)(blob + t.slot_of), ens, nrows, [&](size_t slot, unsigned e, size_t i) { list[slot] = {(unsigned)i, e}; });
}
