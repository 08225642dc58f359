// masked_tables.h -- the host tables of the masked replicas of ONE ensemble (resample.hip: what they are for, and the memo that keeps them per
// selection), built in named steps from the columns' pieces (column_runs.h).  Host code only, no HIP runtime (tests/column_runs_check.cpp).
#pragma once

#include "column_runs.h"

#include <utility>

struct MaskedPlan {
	// key
	size_t mtr = 0, N = 0, first = 0, mtr_local = 0;
	unsigned C = 0, KM = 0, gps = 0;
	bool with_main = false, valid = false, allow_direct = true;
	std::vector<char> sel;
	// products
	unsigned long long gen = 0;
	unsigned W = 0, nstage = 0;
	std::vector<size_t> Kc;
	std::vector<Chunk> runs;            // maximal runs of consecutive traces with one signature (cut at the stage ends), trace order
	std::vector<unsigned> seg_first;    // per stage: the first runs of its segments + the end (nseg + 1 entries), stages concatenated
	std::vector<unsigned> stage_seg0;   // per stage: its first entry in seg_first (nstage + 1)
	std::vector<unsigned> carry;        // per stage: snapshots whose sum is the prefix sum at the stage's start
	std::vector<unsigned> carry_ptr;    // (nstage + 1)
	std::vector<unsigned> trow_ptr;     // rows as signed sums of snapshots: [KM W + 1] pointers, rows in stage / column / group order
	std::vector<unsigned> tidx;
	std::vector<float> tcoef;
	// few columns: the rows straight from the walk -- per run the columns it belongs to and the columns whose group ends with it (+ the rows
	// those sums become)
	bool direct = false, unwritten = false; // unwritten: some row is never stored (an empty group): the row block is cleared first
	std::vector<RunDesc> rdesc;         // the runs with their column bits
	std::vector<unsigned> stage_run0;   // per stage: its first run (nstage + 1)
	std::vector<unsigned> stage_mid;    // per stage: first run of its second segment (== the next stage's first run: one segment)
	std::vector<unsigned> fix_row;      // [nstage][W]: the first row column c stores in the stage's second segment (~0u: none)
	std::vector<unsigned> flush_rows;   // flush destinations (RunDesc::frow points here)
	std::vector<unsigned> rowmap;       // [W][KM]: row of (column, group)
	std::vector<double> Mv;             // trace count per column (replicas: selected traces; plain stack: mtr)
	std::vector<char> blob;             // all device tables in one block: the runs first, offsets of the others below
	size_t o_mv = 0, o_rd = 0, o_tp = 0, o_ti = 0, o_tc = 0, o_map = 0, o_seg = 0, o_car = 0, o_fr = 0, o_fx = 0;
	unsigned row_of(unsigned g, unsigned c) const
	{
		const unsigned g0 = g / gps * gps, ng = std::min(gps, KM - g0);
		return g0 * W + c * ng + (g - g0);
	}
};

// what the steps hand each other (a caller keeps one per host thread)
struct MaskedWork : ColumnWork {
	std::vector<size_t> T;           // end of stage s, local to the shard: one past the last trace that belongs to a group of stage <= s in any column
	std::vector<unsigned> run_stage; // stage of a run
	unsigned sig_of(const MaskedPlan &mp, unsigned r, unsigned c) const { return sig[(size_t)c * mp.runs.size() + r]; } // group of run r in column c
};

// Step 1: the pieces of every column over the WHOLE selection (a trace's group in a replica is its rank among all selected traces, :766),
// their starts in chg, the replicas' trace counts, and the stage ends inside the shard [first, first + mtr_local).
inline void masked_signatures(MaskedPlan &mp, const char *h_sel, MaskedWork &w)
{
	const size_t mtr = mp.mtr, lo = mp.first, hi = mp.first + mp.mtr_local;
	mp.Kc.assign(mp.C, 0);
	w.pieces.resize(mp.W);
	w.chg.assign(mtr + 1, 0);
	w.T.assign(mp.nstage, 0);
	for (unsigned c = 0; c < mp.W; c++) {
		std::vector<Piece> &pc = w.pieces[c];
		const size_t n = column_pieces(c < mp.C ? (const unsigned char *)h_sel + (size_t)c * mtr : nullptr, mtr, mp.KM, pc);
		if (c < mp.C) mp.Kc[c] = n;
		mark_piece_starts(pc, w.chg.data());
		for (size_t q = 0; q < pc.size(); q++) { // [pos, end) with one signature: it ends its stage no earlier than where it ends in the shard
			const size_t end = q + 1 < pc.size() ? pc[q + 1].pos : mtr;
			if (pc[q].v == SIG_DELETED || end <= lo || pc[q].pos >= hi) continue;
			size_t &te = w.T[std::min(pc[q].v, mp.KM - 1) / mp.gps];
			te = std::max(te, std::min(end, hi) - lo);
		}
	}
	for (unsigned sg = 1; sg < mp.nstage; sg++) w.T[sg] = std::max(w.T[sg], w.T[sg - 1]);
	w.T[mp.nstage - 1] = mp.mtr_local; // (traces past the last group of every column change nothing; they ride along)
}

// Step 2: the runs of the shard (local trace indices), cut at signature changes and stage ends; the first run of every stage; the group of
// every run in every column.
inline void masked_runs(MaskedPlan &mp, MaskedWork &w)
{
	const unsigned nstage = mp.nstage;
	mp.runs.clear();
	w.run_stage.clear();
	cut_runs(w.chg.data(), mp.first, mp.first + mp.mtr_local, w.T.data(), nstage, [&](size_t i, unsigned count, unsigned sg) {
		Chunk c; c.t0 = i; c.count = count; c.row = 0;
		mp.runs.push_back(c);
		w.run_stage.push_back(sg);
	});
	const unsigned nr = (unsigned)mp.runs.size();
	mp.stage_run0.assign(nstage + 1, nr);
	for (unsigned r = nr; r-- > 0;) mp.stage_run0[w.run_stage[r]] = r;
	for (unsigned sg = nstage; sg-- > 0;) if (mp.stage_run0[sg] > mp.stage_run0[sg + 1]) mp.stage_run0[sg] = mp.stage_run0[sg + 1]; // (empty stages)
	w.sig.resize((size_t)mp.W * nr);
	for (unsigned c = 0; c < mp.W; c++)
		run_groups(w.pieces[c], nr, [&](size_t r) { return mp.first + (size_t)mp.runs[r].t0; }, w.sig.data() + (size_t)c * nr);
}

// Step 3, few columns: the tables of k_rows_walk / k_seg_fix (stream.hip) -- the runs with their column bits and flush destinations, two
// segments of similar trace counts per stage, and the first row every column stores in the second one (which lacks what the first had collected)
inline void masked_direct_tables(MaskedPlan &mp, const MaskedWork &w)
{
	const unsigned nr = (unsigned)mp.runs.size(), W = mp.W, nstage = mp.nstage;
	mp.rdesc.resize(nr);
	for (unsigned r = 0; r < nr; r++) { RunDesc d; memset(&d, 0, sizeof d); d.t0 = mp.runs[r].t0; d.count = mp.runs[r].count; mp.rdesc[r] = d; }
	mp.unwritten = fill_run_bits(mp.rdesc.data(), nr, w.sig.data(), 0, W, mp.KM, [&](unsigned g, unsigned c) { return mp.row_of(g, c); }, mp.flush_rows);
	mp.stage_mid.assign(nstage, 0); mp.fix_row.assign((size_t)nstage * W, ~0u);
	for (unsigned sg = 0; sg < nstage; sg++) {
		const unsigned q0 = mp.stage_run0[sg], q1 = mp.stage_run0[sg + 1];
		size_t traces = 0, done = 0;
		for (unsigned r = q0; r < q1; r++) traces += mp.runs[r].count;
		unsigned qm = q1;
		for (unsigned r = q0; r < q1; r++) { if (r > q0 && 2 * done >= traces) { qm = r; break; } done += mp.runs[r].count; }
		mp.stage_mid[sg] = qm;
		for (unsigned r = qm; r < q1; r++) {
			unsigned fr = mp.rdesc[r].frow;
			for (unsigned c = 0; c < W; c++)
				if ((mp.rdesc[r].flush >> c) & 1u) { if (mp.fix_row[(size_t)sg * W + c] == ~0u) mp.fix_row[(size_t)sg * W + c] = mp.flush_rows[fr]; fr++; }
		}
	}
}

// Step 3, many columns: the tables of k_prefix_walk / k_combine_terms (stream.hip) -- every stage's runs in up to want_seg segments of
// similar trace counts, each walked by its own workgroups; the carries; every row as a signed sum of snapshots
inline void masked_snapshot_tables(MaskedPlan &mp, const MaskedWork &w, unsigned want_seg)
{
	const unsigned nr = (unsigned)mp.runs.size(), W = mp.W, nstage = mp.nstage, KM = mp.KM;
	std::vector<unsigned> seg_of(nr, 0), seg_last;        // segment (global numbering) of a run; last run of a segment
	std::vector<unsigned> seg_stage_first(nstage + 1, 0); // first global segment of a stage
	for (unsigned sg = 0; sg < nstage; sg++) {
		const unsigned r = mp.stage_run0[sg], r1 = mp.stage_run0[sg + 1];
		mp.stage_seg0[sg] = (unsigned)mp.seg_first.size();
		seg_stage_first[sg] = (unsigned)seg_last.size();
		size_t traces = 0, done = 0;
		for (unsigned q = r; q < r1; q++) traces += mp.runs[q].count;
		const unsigned nseg = std::min(want_seg, r1 - r);
		unsigned k = 0;
		for (unsigned q = r; q < r1; q++) {
			// run q opens segment k when the traces before it reach k / nseg of the stage
			if (k < nseg && (q == r || done * nseg >= (size_t)k * traces)) {
				if (q != r) seg_last.push_back(q - 1);
				mp.seg_first.push_back(q);
				k++;
			}
			seg_of[q] = (unsigned)(seg_stage_first[sg] + k - 1);
			done += mp.runs[q].count;
		}
		if (r1 > r) seg_last.push_back(r1 - 1);
		mp.seg_first.push_back(r1);
	}
	mp.stage_seg0[nstage] = (unsigned)mp.seg_first.size();
	seg_stage_first[nstage] = (unsigned)seg_last.size();
	// prefix sum at the start of a stage = sum of the final snapshots of the segments of the last non-empty stage before it
	std::vector<unsigned> cur;
	for (unsigned sg = 0; sg < nstage; sg++) {
		mp.carry_ptr[sg] = (unsigned)mp.carry.size();
		mp.carry.insert(mp.carry.end(), cur.begin(), cur.end());
		if (seg_stage_first[sg + 1] > seg_stage_first[sg]) cur.assign(seg_last.begin() + seg_stage_first[sg], seg_last.begin() + seg_stage_first[sg + 1]);
	}
	mp.carry_ptr[nstage] = (unsigned)mp.carry.size();
	// G(k) = sum of all traces before run k, as a signed sum of snapshots: snap[k - 1] + the final snapshots of the earlier segments
	// of the same stage (segment 0 of a stage starts from the carried prefix: its snapshots are global)
	auto add_G = [&](std::vector<std::pair<unsigned, int>> &terms, unsigned k, int sign) {
		if (!k) return;
		const unsigned r = k - 1, sg = w.run_stage[r];
		terms.emplace_back(r, sign);
		for (unsigned q = seg_stage_first[sg]; q < seg_of[r]; q++) terms.emplace_back(seg_last[q], sign);
	};
	// rows: for every column and group the maximal stretches [a, b) of consecutive runs that belong to it: sum of G(b) - G(a)
	const unsigned nrow = KM * W;
	std::vector<std::vector<std::pair<unsigned, int>>> lists(nrow);
	for (unsigned c = 0; c < W; c++) {
		unsigned a = 0, cur_g = SIG_DELETED;
		for (unsigned r = 0; r <= nr; r++) {
			const unsigned g = r < nr ? w.sig_of(mp, r, c) : SIG_DELETED;
			if (g == cur_g) continue;
			if (cur_g != SIG_DELETED) { auto &L = lists[mp.row_of(std::min(cur_g, KM - 1), c)]; add_G(L, r, +1); add_G(L, a, -1); }
			cur_g = g; a = r;
		}
	}
	for (unsigned r = 0; r < nrow; r++) {
		mp.trow_ptr[r] = (unsigned)mp.tidx.size();
		auto &L = lists[r];
		std::sort(L.begin(), L.end());
		for (size_t i = 0; i < L.size();) { // merge equal snapshots, drop what cancels
			size_t j = i; int cf = 0;
			while (j < L.size() && L[j].first == L[i].first) cf += L[j++].second;
			if (cf) { mp.tidx.push_back(L[i].first); mp.tcoef.push_back((float)cf); }
			i = j;
		}
	}
	mp.trow_ptr[nrow] = (unsigned)mp.tidx.size();
}

// the first n elements of v as the next array of the block; returns its offset
template <class T>
inline size_t table_put(TableLayout &lay, std::vector<char> &blob, const std::vector<T> &v, size_t n)
{
	const size_t o = lay.add<T>(n);
	blob.resize(lay.bytes, 0);
	if (n) memcpy(blob.data() + o, v.data(), n * sizeof(T));
	return o;
}

// Step 4: the row map, the columns' trace counts, and everything the kernels read in ONE block -- one host-to-device copy per new selection.
// The 16-byte records first (runs at offset 0: the snapshot form only; run descriptors), then the doubles, then the words.
inline void masked_pack(MaskedPlan &mp)
{
	const unsigned W = mp.W, KM = mp.KM;
	mp.rowmap.assign((size_t)W * KM, 0);
	for (unsigned c = 0; c < W; c++) for (unsigned g = 0; g < KM; g++) mp.rowmap[(size_t)c * KM + g] = mp.row_of(g, c);
	mp.Mv.assign(W, 0.0);
	for (unsigned c = 0; c < mp.C; c++) mp.Mv[c] = (double)mp.Kc[c];
	if (mp.with_main) mp.Mv[mp.C] = (double)(unsigned)mp.mtr;
	static_assert(sizeof(Chunk) == 16 && sizeof(RunDesc) == 32, "the records keep the block's 16-byte alignment");
	TableLayout lay;
	mp.blob.clear();
	table_put(lay, mp.blob, mp.runs, mp.direct ? 0 : mp.runs.size());
	mp.o_rd = table_put(lay, mp.blob, mp.rdesc, mp.rdesc.size());
	mp.o_mv = table_put(lay, mp.blob, mp.Mv, W);
	mp.o_tp = table_put(lay, mp.blob, mp.trow_ptr, mp.trow_ptr.size());
	mp.o_ti = table_put(lay, mp.blob, mp.tidx, mp.tidx.size());
	mp.o_tc = table_put(lay, mp.blob, mp.tcoef, mp.tcoef.size());
	mp.o_map = table_put(lay, mp.blob, mp.rowmap, mp.rowmap.size());
	mp.o_seg = table_put(lay, mp.blob, mp.seg_first, mp.seg_first.size());
	mp.o_car = table_put(lay, mp.blob, mp.carry, mp.carry.size());
	mp.o_fr = table_put(lay, mp.blob, mp.flush_rows, mp.flush_rows.size());
	mp.o_fx = table_put(lay, mp.blob, mp.fix_row, mp.fix_row.size());
	mp.blob.resize(std::max<size_t>(mp.blob.size(), 4), 0); // (never an empty block)
}

// segments per stage of the snapshot form: ~seg_wgs workgroups over the bx blocks of 1024 samples
inline unsigned masked_want_seg(size_t N, unsigned seg_wgs) { return std::max(1u, seg_wgs / std::max(1u, (unsigned)((N + 1023) / 1024))); }

// The tables of a selection sel[C][mtr] for the shard [first, first + mtr_local) of its traces (local trace indices): KM groups in stages of
// gps, the plain stack as column C (with_main); `direct`: the rows straight from the walk (at most 16 columns), else the snapshot form with
// up to want_seg segments per stage.  The caller owns the key's remaining fields (N, sel, gen, valid).
inline void masked_build(MaskedPlan &mp, MaskedWork &w, size_t mtr, const char *h_sel, unsigned C, unsigned KM, bool with_main, unsigned gps, bool direct,
                         unsigned want_seg, size_t first, size_t mtr_local)
{
	mp.mtr = mtr; mp.C = C; mp.KM = KM; mp.gps = gps; mp.with_main = with_main; mp.first = first; mp.mtr_local = mtr_local;
	mp.W = C + (with_main ? 1u : 0u);
	mp.nstage = (KM + gps - 1) / gps;
	mp.direct = direct; mp.unwritten = false;
	mp.rdesc.clear(); mp.flush_rows.clear(); mp.stage_mid.clear(); mp.fix_row.clear();
	mp.seg_first.clear(); mp.stage_seg0.assign(mp.nstage + 1, 0); mp.carry.clear(); mp.carry_ptr.assign(mp.nstage + 1, 0);
	mp.trow_ptr.assign((size_t)KM * mp.W + 1, 0); mp.tidx.clear(); mp.tcoef.clear();
	masked_signatures(mp, h_sel, w);
	masked_runs(mp, w);
	if (direct) masked_direct_tables(mp, w);
	else masked_snapshot_tables(mp, w, want_seg);
	masked_pack(mp);
}
