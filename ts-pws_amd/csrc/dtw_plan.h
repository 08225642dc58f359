// dtw_plan.h -- how tspws_hip_dtw_rows (dtw_rows.hip) cuts its work: the parameter and range checks, the lags per lane, the samples and the
// choice-plane words of every lag range with their offsets, the LDS of a wave, the rounds of whole ensembles that keep the choice planes inside
// the parts budget, and the ONE table block a round uploads.  Host code only, no HIP runtime: tests/dtw_plan_check.cpp compiles it with a plain
// C++17 compiler.
//
// LAGS.  nl = 2 Lmax + 1 lags l = -Lmax .. Lmax, lag index li = l + Lmax.  One wave takes a (row, range); lane j holds the Q consecutive lag
// indices j Q .. j Q + Q - 1, Q = 1, 2 or 4 the smallest with 64 Q >= nl; nlp = 64 Q > nl: there is always at least one pad index, the last
// lane's last.
// SAMPLES.  Range w = [n0, n1) holds n_w = n1 - n0 <= DT_NMAX samples; the lags of a row lie range after range: those of range w in
// [off[w], off[w + 1]), T = off[W].
// CHOICE PLANES.  Two bits per (sample, lag index): 0 = C, 1 = Mn, 2 = Pl (sample 0 has none: 0).  Sixteen samples per 32-bit word, sample i in
// the bits 2 (i % 16) of word i / 16; the plane of (row, range w) is words[w] = ceil(n_w / 16) rows of nlp words, [word][lag index].  A
// participating row's planes lie range after range: range w at poff[w] words into its P = poff[W] words; slot s of the round at s P.
// ROUNDS.  Whole ensembles whose participating rows' planes and table stay inside the parts budget; the first ensemble of a round is always
// taken (one alone may exceed the budget).  The round rule, participation, the slots and the range words are host_plan.h's.
#pragma once

#include "host_plan.h"

#include <cstdint>

enum { DT_WMAX = 4, DT_LMAX = 127, DT_BMAX = 8, DT_NMAX = 131072, DT_CHUNK = 64, DT_BACK = 8 }; // ..., samples per staged chunk, words per backtrack block

struct DtwPar { unsigned Lmax, b; }; // (tspws_dtw_par)

// what is wrong with the parameters (NULL: nothing); needs no plan
inline const char *dt_par_error(const DtwPar &p)
{
	if (p.Lmax < 1 || p.Lmax > DT_LMAX) return "a largest lag outside [1, 127]";
	if (p.b < 1 || p.b > DT_BMAX) return "a strain limit outside [1, 8]";
	return nullptr;
}

// what is wrong with the W ranges win[2 w], win[2 w + 1] (NULL: nothing); needs no plan (n1 <= N is the caller's check)
inline const char *dt_range_error(const size_t *win, unsigned W)
{
	if (const char *e = range_error(win, W, LAG_RANGES)) return e;
	for (unsigned w = 0; w < W; w++)
		if (win[2 * w + 1] - win[2 * w] > DT_NMAX) return "a lag range longer than 131072 samples";
	return nullptr;
}

struct DtwGeom {
	unsigned nl, Q, nlp, W;
	unsigned n0[DT_WMAX], n[DT_WMAX];        // first sample and samples of range w (0 past W)
	unsigned off[DT_WMAX + 1];               // the lags of range w: [off[w], off[w + 1]); T = off[W] (and past W)
	unsigned words[DT_WMAX];                 // choice words per lag index of range w
	unsigned long long poff[DT_WMAX + 1];    // the plane of range w: [poff[w], poff[w + 1]) words of the row's planes; P = poff[W]
	unsigned T() const { return off[DT_WMAX]; }
	unsigned long long P() const { return poff[DT_WMAX]; }
};

// (parameters and ranges checked by the caller; n1 <= N < 2^32)
inline DtwGeom dt_geom(const DtwPar &p, const size_t *win, unsigned W)
{
	DtwGeom g{};
	g.nl = 2 * p.Lmax + 1;
	g.Q = g.nl <= 64 ? 1 : g.nl <= 128 ? 2 : 4;
	g.nlp = 64 * g.Q;
	g.W = W;
	for (unsigned w = 0; w < DT_WMAX; w++) {
		if (w < W) {
			g.n0[w] = (unsigned)win[2 * w];
			g.n[w] = (unsigned)(win[2 * w + 1] - win[2 * w]);
			g.words[w] = (g.n[w] + 15) / 16;
		}
		g.off[w + 1] = g.off[w] + g.n[w];
		g.poff[w + 1] = g.poff[w] + (unsigned long long)g.words[w] * g.nlp;
	}
	return g;
}

// the LDS of a wave in bytes.  Forward: the rings D[b][Q][64] and e[b - 1][Q][64] (none for b == 1), then twice (a chunk in use, one being
// filled) the normalised row samples [64] and the normalised reference reach [64 + 64 Q] (64 + 2 Lmax in use).  Backward, over the same bytes:
// a block of DT_BACK choice words [DT_BACK][nlp], then the lags of its 16 DT_BACK samples.
struct DtwLds { unsigned ringD, ringE, stage, stage_doubles, back_words, back_lags, bytes; }; // offsets in bytes
inline DtwLds dt_lds(const DtwPar &p, unsigned Q)
{
	DtwLds o;
	const unsigned ring = p.b > 1 ? 64 * Q * 8 : 0;
	o.ringD = 0;
	o.ringE = o.ringD + p.b * ring;
	o.stage = o.ringE + (p.b - 1) * ring;
	o.stage_doubles = DT_CHUNK + DT_CHUNK + 64 * Q;
	const unsigned fwd = o.stage + 2 * o.stage_doubles * 8;
	o.back_words = 0;
	o.back_lags = DT_BACK * 64 * Q * 4;
	const unsigned back = o.back_lags + 16 * DT_BACK * 4;
	o.bytes = std::max(fwd, back);
	return o;
}

// the table block of a round: slot of every (ensemble of the round, m) or NOSLOT
struct DtwTab { size_t slot_of, bytes; };
inline DtwTab dt_tab(size_t nall)
{
	TableLayout lay;
	DtwTab t;
	t.slot_of = lay.add<unsigned>(nall);
	t.bytes = lay.bytes;
	return t;
}

inline size_t dt_plane_bytes(size_t nrows, const DtwGeom &g) { return nrows * (size_t)g.P() * sizeof(unsigned); }
// nrows0: participating_rows0
inline size_t dt_round_bytes(const size_t *nrows0, size_t j0, size_t j1, size_t M, const DtwGeom &g)
{
	return dt_plane_bytes(nrows0[j1] - nrows0[j0], g) + dt_tab((j1 - j0) * M).bytes;
}

inline std::vector<Round> dt_rounds(size_t B, const size_t *nrows0, size_t M, const DtwGeom &g, size_t budget)
{
	return whole_ensemble_rounds(B, [&](size_t j0, size_t j1) { return dt_round_bytes(nrows0, j0, j1, M, g) <= budget; });
}

// the table of round r into blob (dt_tab's layout with the round's own counts; zeroed by the caller); returns the participating rows
inline size_t dt_fill_round(char *blob, const DtwTab &t, const Round &r, size_t M, const unsigned *h_mtr)
{
	return fill_round_slots((unsigned *)(blob + t.slot_of), r, M, h_mtr, [](size_t, size_t, size_t) {});
}
