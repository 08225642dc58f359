// column_runs.h -- which trace lands in which partial-stack row of the two-stage replicas: the ONE host definition that the masked replicas
// of a single ensemble (masked_tables.h, resample.hip) and the batched two-stage jackknife (jk_batch_two_stage.hip) build their run tables from.
// Host code only, no HIP runtime: tests/column_runs_check.cpp compiles it with a plain C++17 compiler.
//
// A COLUMN is a replica (a row of the selection, byte 1 = the trace is kept) or the plain stack.  The signature rule, stated once:
//   replica      the group of a kept trace is floor(k KM / max(K_c, 1)), k = its rank among the column's kept traces, K_c = their number
//                (ts_pws1f_lib.c:758-772; the integer quotient is the reference's floor of the double quotient: k KM < 2^53 and a non-integer
//                quotient is at least 1 / K_c away from the next integer); any other byte: SIG_DELETED, the trace is not in the replica
//   plain stack  min(floor(i KM / m), KM - 1) for trace i of m (:876)
// A column's signature is piecewise constant, so it is kept as PIECES (start, signature) and never trace by trace; the traces are cut into RUNS at
// the starts of all columns' pieces, and a run has one signature in every column.  Groups ascend along a column.
#pragma once

#include "host_plan.h" // TableLayout (the layout of the run tables' blocks)

#include <cstring>

struct Chunk { // one streaming work item of the partial-stack kernel
	unsigned long long t0; // first local trace
	unsigned count;        // traces
	unsigned row;          // destination row (group / class)
};

struct RunDesc { // one run of consecutive traces with one signature, for k_rows_walk (stream.hip)
	unsigned long long t0;   // first trace
	unsigned count;          // traces
	unsigned member, flush;  // bit c: the run belongs to column c / column c's group ends with this run
	unsigned frow;           // first entry of the run's flush destinations in flush_rows (ascending column order)
	unsigned pad[2];
};

constexpr unsigned SIG_DELETED = ~0u; // (32-bit signatures: Kmax is an unsigned in t_tsPWS, any value is a legal group count)
constexpr unsigned RUN_MAX = 0xFFFFFFF0u; // traces of a run: a longer one is cut

struct Piece { size_t pos; unsigned v; }; // a column has signature v from trace pos on, up to the next piece

// The pieces of one column of m traces; returns K_c (row == NULL, the plain stack: m).  A replica's signature changes where the selection
// byte changes and, inside a stretch of kept traces, where the group steps; the stretches are found a machine word at a time (deleted ones
// by memchr), the steps by ONE division per step (<= KM per column): the plain stack's are at ceil(g m / KM).
inline size_t column_pieces(const unsigned char *row, size_t m, unsigned KM, std::vector<Piece> &pc)
{
	pc.clear();
	auto emit = [&](size_t pos, unsigned v) {
		if (!pc.empty() && pc.back().v == v) return; // (no change after all)
		pc.push_back(Piece{pos, v});
	};
	if (!row) {
		emit(0, 0);
		for (unsigned long long g = 1; g < KM; g++) {
			const unsigned long long pos = (g * m + KM - 1) / KM;
			if (pos >= m) break;
			emit((size_t)pos, (unsigned)(pos * KM / m));
		}
		return m;
	}
	size_t n = 0;
	for (size_t i = 0; i < m; i++) n += row[i] == 1; // (vectorised)
	const unsigned long long Kc = std::max<size_t>(n, 1);
	unsigned long long k = 0, g = 0, kb = (Kc + KM - 1) / KM; // rank among the kept traces; its group; the rank at which the group steps next
	size_t i = 0;
	if (m && row[0] != 1) emit(0, SIG_DELETED);
	while (i < m) {
		if (row[i] != 1) { // a stretch that is not kept: up to the next byte 1
			const void *q = memchr(row + i, 1, m - i);
			i = q ? (size_t)((const unsigned char *)q - row) : m;
			continue;
		}
		size_t j = i; // a stretch of kept traces [i, j): words of eight bytes 1, then the tail
		while (j + 8 <= m) { unsigned long long w; memcpy(&w, row + j, 8); if (w != 0x0101010101010101ull) break; j += 8; }
		while (j < m && row[j] == 1) j++;
		const unsigned long long k1 = k + (j - i);
		if (kb <= k) { g = k * KM / Kc; kb = ((g + 1) * Kc + KM - 1) / KM; }
		emit(i, (unsigned)g);
		while (kb < k1) { // the group steps inside the stretch
			const size_t pos = i + (size_t)(kb - k);
			g = kb * KM / Kc; kb = ((g + 1) * Kc + KM - 1) / KM;
			emit(pos, (unsigned)g);
		}
		k = k1;
		if (j < m) emit(j, SIG_DELETED);
		i = j;
	}
	return n;
}

// chg[i] = 1: a piece of the column starts at trace i, so trace i starts a run
inline void mark_piece_starts(const std::vector<Piece> &pc, unsigned char *chg)
{
	for (const Piece &q : pc) chg[q.pos] = 1;
}

// Traces [lo, hi) in runs: a run ends before the next marked start (chg, indexed like the pieces) and at the limits lim[0 .. nlim) (ascending,
// relative to lo; the last limit counts as hi - lo; none: no further cut), and holds at most RUN_MAX traces.  emit(first trace relative to lo,
// traces, index of the limit the run lies under).
template <class Emit>
inline void cut_runs(const unsigned char *chg, size_t lo, size_t hi, const size_t *lim, unsigned nlim, Emit emit)
{
	const size_t n = hi - lo;
	unsigned s = 0;
	for (size_t i = 0; i < n;) {
		while (s + 1 < nlim && i >= lim[s]) s++;
		const size_t end = s + 1 < nlim ? std::min(n, lim[s]) : n;
		size_t j = i + 1;
		if (j < end) { // the next trace that starts a run (bytes of chg: memchr)
			const void *q = memchr(chg + lo + j, 1, end - j);
			j = q ? (size_t)((const unsigned char *)q - chg) - lo : end;
		}
		if (j - i > RUN_MAX) j = i + RUN_MAX;
		emit(i, (unsigned)(j - i), s);
		i = j;
	}
}

// sig[r] = the column's group in run r of nr: the piece that holds the run's first trace t0(r) (pieces and runs are both in trace order)
template <class T0>
inline void run_groups(const std::vector<Piece> &pc, size_t nr, T0 t0, unsigned *sig)
{
	size_t q = 0;
	for (size_t r = 0; r < nr; r++) {
		const size_t t = t0(r);
		while (q + 1 < pc.size() && pc[q + 1].pos <= t) q++;
		sig[r] = pc.empty() ? SIG_DELETED : pc[q].v;
	}
}

// member, flush and frow of the runs R[0 .. nr) for columns [c0, c1) (bit c - c0; at most 32 columns), from sig[(c - c0) nr + r].  Column by
// column from the last run back: a run that belongs to the column ends the column's group when the next run that belongs to it has another
// group (or there is none).  Then the flush destinations row_of(group, column) of every run, in ascending column order, behind flush_rows.
// Returns whether some (column, group) is never stored (groups ascend along a column: one that stores fewer than KM rows misses one).
template <class RowOf>
inline bool fill_run_bits(RunDesc *R, size_t nr, const unsigned *sig, unsigned c0, unsigned c1, unsigned KM, RowOf row_of, std::vector<unsigned> &flush_rows)
{
	bool unwritten = false;
	for (unsigned c = c0; c < c1; c++) {
		const unsigned *sg = sig + (size_t)(c - c0) * nr;
		unsigned next_g = SIG_DELETED, stored = 0;
		for (size_t r = nr; r-- > 0;) {
			const unsigned g = sg[r];
			if (g == SIG_DELETED) continue;
			R[r].member |= 1u << (c - c0);
			if (g != next_g) { R[r].flush |= 1u << (c - c0); stored++; }
			next_g = g;
		}
		if (stored < KM) unwritten = true;
	}
	for (size_t r = 0; r < nr; r++) {
		R[r].frow = (unsigned)flush_rows.size();
		for (unsigned c = c0; c < c1; c++)
			if ((R[r].flush >> (c - c0)) & 1u) flush_rows.push_back(row_of(std::min(sig[(size_t)(c - c0) * nr + r], KM - 1), c));
	}
	return unwritten;
}

// scratch of the builders (a caller keeps one per host thread)
struct ColumnWork {
	std::vector<std::vector<Piece>> pieces; // per column
	std::vector<unsigned char> chg;         // chg[i]: trace i starts a run
	std::vector<unsigned> sig;              // [column][run]
};

// Runs, column bits and flush destinations of columns [c0, c1) of one ensemble of m traces, for a walk that keeps those columns' running sums
// (k_jb2_rows_walk): sel(c) = the column's selection row (NULL: the plain stack), Kc[c] = its kept traces.  The runs (t0 = base + trace) go
// behind `runs`, the destinations row_of(group, column) behind `flush_rows`; returns whether some row of these columns is never stored.
template <class Sel, class RowOf>
inline bool tile_runs(ColumnWork &w, size_t m, unsigned KM, unsigned c0, unsigned c1, Sel sel, RowOf row_of, unsigned long long base, unsigned *Kc,
                      std::vector<RunDesc> &runs, std::vector<unsigned> &flush_rows)
{
	if (w.pieces.size() < c1 - c0) w.pieces.resize(c1 - c0);
	w.chg.assign(m + 1, 0);
	for (unsigned c = c0; c < c1; c++) {
		const unsigned char *row = sel(c);
		const size_t n = column_pieces(row, m, KM, w.pieces[c - c0]);
		if (row) Kc[c] = (unsigned)n;
		mark_piece_starts(w.pieces[c - c0], w.chg.data());
	}
	const size_t run0 = runs.size();
	cut_runs(w.chg.data(), 0, m, nullptr, 0, [&](size_t i, unsigned count, unsigned) {
		RunDesc d;
		memset(&d, 0, sizeof d);
		d.t0 = base + i; d.count = count;
		runs.push_back(d);
	});
	const size_t nr = runs.size() - run0;
	RunDesc *R = runs.data() + run0;
	w.sig.resize((size_t)(c1 - c0) * nr);
	for (unsigned c = c0; c < c1; c++)
		run_groups(w.pieces[c - c0], nr, [&](size_t r) { return (size_t)(R[r].t0 - base); }, w.sig.data() + (size_t)(c - c0) * nr);
	return fill_run_bits(R, nr, w.sig.data(), c0, c1, KM, row_of, flush_rows);
}
