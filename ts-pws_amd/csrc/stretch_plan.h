// stretch_plan.h -- how tspws_hip_stretch_rows (stretch_rows.hip) cuts its work: the packed window columns and their segments, the rounds of
// (whole ensembles x chunks of the stretch grid) that keep the stretched references and the partial sums inside the parts budget, and the ONE
// table block a round uploads.  Host code only, no HIP runtime: tests/stretch_plan_check.cpp compiles it with a plain C++17 compiler.
//
// COLUMNS.  The samples of the W windows [n0_w, n1_w) are laid side by side, every window padded to a multiple of 4 columns (the pad columns of
// the stretched references are zero), and every window is cut into SEGMENTS of SR_SEG samples counted from ITS first sample -- so the segments
// of a window, and with them the order of every sum over it, depend on that window alone.  Segment s holds the samples [n0, n0 + len) of window
// w in the packed columns [joff, joff + plen), plen = len rounded up to 4; joff is a multiple of 4.
// ROUNDS.  A round is the ensembles [j0, j1) and walks the padded grid (Epad = E rounded up to 16) in chunks of Ec stretches, Ec a multiple
// of 16.  What a round holds at a time: the partial sums of all its participating rows over the whole grid, the S^2 partial sums, its table
// (together: the fixed part) and the stretched references of ONE chunk.  The first ensemble of a round is always taken with Ec >= 16 (one
// ensemble x 16 stretches may exceed the budget on its own); the round extends while the fixed part and a chunk of 16 still fit; then Ec is
// the largest multiple of 16 that fits.  The round rule, participation and the slots are host_plan.h's.
#pragma once

#include "host_plan.h"

#include <cstdint>

enum { SR_SEG = 512, SR_ET = 16, SR_ROWS = 32, SR_WMAX = 4, SR_EMAX = 4096 }; // samples per segment, stretches per tile, rows per wave tile

struct SrSeg { unsigned long long n0, joff; unsigned len, plen, w, pad; };
// up to SR_ROWS participating rows of ensemble b (bl: its index in the round): their partial-sum slots, and their row numbers in the list, start at slot0
struct SrTile { unsigned b, bl, count, pad; unsigned long long slot0; };

struct SrCols {
	std::vector<SrSeg> segs;
	unsigned seg0[SR_WMAX + 1] = {0, 0, 0, 0, 0}; // the segments of window w: [seg0[w], seg0[w + 1])
	size_t J = 0;                                // packed columns
};

// win = W pairs [n0, n1), n0 < n1 (checked by the caller), 1 <= W <= SR_WMAX
inline SrCols sr_columns(const size_t *win, unsigned W)
{
	SrCols c;
	for (unsigned w = 0; w < W; w++) {
		c.seg0[w] = (unsigned)c.segs.size();
		for (size_t n = win[2 * w]; n < win[2 * w + 1]; n += SR_SEG) {
			SrSeg s;
			s.n0 = n; s.joff = c.J; s.len = (unsigned)std::min<size_t>(SR_SEG, win[2 * w + 1] - n); s.plen = (s.len + 3u) & ~3u; s.w = w; s.pad = 0;
			c.J += s.plen;
			c.segs.push_back(s);
		}
	}
	for (unsigned w = W; w <= SR_WMAX; w++) c.seg0[w] = (unsigned)c.segs.size();
	return c;
}

inline unsigned sr_epad(unsigned E) { return (E + SR_ET - 1) / SR_ET * SR_ET; }

// the table block of a round: segments | the padded grid | tiles | participating rows (m) | slot of every (ensemble of the round, m) or NOSLOT
struct SrTab { size_t segs, eps, tiles, list, slot_of, bytes; };
inline SrTab sr_tab(size_t nseg, size_t epad, size_t ntiles, size_t nlist, size_t nall)
{
	TableLayout lay;
	SrTab t;
	t.segs = lay.add<SrSeg>(nseg); t.eps = lay.add<double>(epad); t.tiles = lay.add<SrTile>(ntiles); t.list = lay.add<unsigned>(nlist);
	t.slot_of = lay.add<unsigned>(nall);
	t.bytes = lay.bytes;
	return t;
}

// the device blocks of a round, in doubles: dots[slot][seg][epad], xx[slot][seg], ss[bl][epad][seg] in one block; S[bl][Ec][J] in another
struct SrPart { size_t dots, xx, ss, doubles; };
inline SrPart sr_part(size_t nb, size_t nrows, size_t nseg, size_t epad)
{
	SrPart p;
	p.dots = 0; p.xx = nrows * nseg * epad; p.ss = p.xx + nrows * nseg; p.doubles = p.ss + nb * epad * nseg;
	return p;
}
inline size_t sr_s_bytes(size_t nb, size_t Ec, size_t J) { return nb * Ec * J * sizeof(double); }

struct SrRound : Round { unsigned Ec, nchunks; };

// nrows0: participating_rows0; tiles of an ensemble: ceil(rows / SR_ROWS)
inline size_t sr_tiles(const size_t *nrows0, size_t j0, size_t j1)
{
	size_t n = 0;
	for (size_t b = j0; b < j1; b++) n += (nrows0[b + 1] - nrows0[b] + SR_ROWS - 1) / SR_ROWS;
	return n;
}
inline size_t sr_fixed_bytes(const size_t *nrows0, size_t j0, size_t j1, size_t M, unsigned E, const SrCols &c)
{
	const size_t nb = j1 - j0, nrows = nrows0[j1] - nrows0[j0], epad = sr_epad(E);
	return sr_part(nb, nrows, c.segs.size(), epad).doubles * sizeof(double) + sr_tab(c.segs.size(), epad, sr_tiles(nrows0, j0, j1), nrows, nb * M).bytes;
}

inline std::vector<SrRound> sr_rounds(size_t B, const size_t *nrows0, size_t M, unsigned E, const SrCols &c, size_t budget)
{
	std::vector<SrRound> rounds;
	const unsigned epad = sr_epad(E);
	auto fits = [&](size_t j0, size_t j1, size_t Ec) {
		const size_t f = sr_fixed_bytes(nrows0, j0, j1, M, E, c), s = sr_s_bytes(j1 - j0, Ec, c.J);
		return f <= budget && s <= budget - f;
	};
	for (const Round &r : whole_ensemble_rounds(B, [&](size_t j0, size_t j1) { return fits(j0, j1, SR_ET); })) {
		unsigned Ec = SR_ET;
		while (Ec < epad && fits(r.j0, r.j1, Ec + SR_ET)) Ec += SR_ET;
		rounds.push_back({r, Ec, (epad + Ec - 1) / Ec});
	}
	return rounds;
}

// the table of round r into blob (sr_tab's layout with the round's own counts; zeroed by the caller); returns the participating rows
inline size_t sr_fill_round(char *blob, const SrTab &t, const SrRound &r, size_t M, const unsigned *h_mtr, const SrCols &c, const double *eps, unsigned E)
{
	SrSeg *segs = (SrSeg *)(blob + t.segs);
	double *ep = (double *)(blob + t.eps);
	SrTile *tiles = (SrTile *)(blob + t.tiles);
	unsigned *list = (unsigned *)(blob + t.list), *slot_of = (unsigned *)(blob + t.slot_of);
	for (size_t s = 0; s < c.segs.size(); s++) segs[s] = c.segs[s];
	const unsigned epad = sr_epad(E);
	for (unsigned e = 0; e < epad; e++) ep[e] = e < E ? eps[e] : 0.0; // (the pad stretches are never evaluated: their columns of S are zero)
	size_t nt = 0;
	return fill_round_slots(slot_of, r, M, h_mtr, [&](size_t slot, size_t b, size_t m) {
		list[slot] = (unsigned)m;
		if (!nt || tiles[nt - 1].b != b || tiles[nt - 1].count == SR_ROWS) tiles[nt++] = {(unsigned)b, (unsigned)(b - r.j0), 0, 0, slot}; // the next tile of ensemble b
		tiles[nt - 1].count++;
	});
}
