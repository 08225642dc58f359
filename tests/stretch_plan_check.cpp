// stretch_plan_check.cpp -- csrc/stretch_plan.h against a direct enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// stretch_plan_check` with AddressSanitizer + UBSan; tests/test_stretch_plan_cpu.py runs it).  It requires:
//   columns  every sample of every window lies in exactly one segment, at the packed column joff + (n - n0); the segments of a window start
//            at n0_w + k SR_SEG (they depend on that window alone) and hold at most SR_SEG samples; joff and plen are multiples of 4,
//            len <= plen < len + 4; the packed ranges tile [0, J) in order; seg0 brackets each window's segments
//   rounds   the rounds tile the ensembles in order; Ec is a multiple of 16 in [16, Epad] and nchunks chunks just cover Epad; every
//            (ensemble, stretch) falls into exactly one (round, chunk); the fixed part and one chunk of S stay within the budget unless the
//            round is one ensemble at Ec = 16; a round that stops early could not have taken the next ensemble, an Ec below Epad could not grow
//   table    every array of the block lies inside it, aligned, none overlapping (the block is allocated at its exact size: ASan sees any
//            write past it); the tiles hold each participating row of each ensemble exactly once, in ascending order, at most SR_ROWS each,
//            with consecutive slots; slot_of inverts the list and marks the rows left out; the grid is copied and padded
#include "stretch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

static unsigned long long nchecks = 0;
#define REQUIRE(c)                                                                 \
	do {                                                                           \
		nchecks++;                                                                 \
		if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
	} while (0)

static void check_columns(const std::vector<size_t> &win, size_t N)
{
	const unsigned W = (unsigned)(win.size() / 2);
	const SrCols c = sr_columns(win.data(), W);
	size_t J = 0, s = 0;
	for (unsigned w = 0; w < W; w++) {
		REQUIRE(c.seg0[w] == s);
		std::vector<unsigned char> seen(N, 0);
		const size_t n0 = win[2 * w], n1 = win[2 * w + 1];
		for (size_t k = 0; n0 + k * SR_SEG < n1; k++, s++) {
			REQUIRE(s < c.segs.size());
			const SrSeg &g = c.segs[s];
			REQUIRE(g.w == w && g.n0 == n0 + k * SR_SEG && g.len >= 1 && g.len <= SR_SEG && g.n0 + g.len <= n1);
			REQUIRE(g.joff == J && g.joff % 4 == 0 && g.plen % 4 == 0 && g.plen >= g.len && g.plen < g.len + 4);
			for (size_t n = g.n0; n < g.n0 + g.len; n++) { REQUIRE(n < N && !seen[n]); seen[n] = 1; }
			J += g.plen;
		}
		for (size_t n = 0; n < N; n++) REQUIRE(seen[n] == (n >= n0 && n < n1));
	}
	for (unsigned w = W; w <= SR_WMAX; w++) REQUIRE(c.seg0[w] == c.segs.size());
	REQUIRE(s == c.segs.size() && J == c.J);
}

static void check_rounds(size_t B, size_t M, unsigned E, const std::vector<unsigned> *mtr, const SrCols &c, size_t budget, const std::vector<double> &eps)
{
	std::vector<size_t> nrows0(B + 1, 0);
	for (size_t b = 0; b < B; b++) {
		size_t n = M;
		if (mtr) { n = 0; for (size_t m = 0; m < M; m++) n += (*mtr)[b * M + m] > 0; }
		nrows0[b + 1] = nrows0[b] + n;
	}
	const unsigned epad = sr_epad(E);
	REQUIRE(epad % 16 == 0 && epad >= E && epad < E + 16);
	const std::vector<SrRound> rounds = sr_rounds(B, nrows0.data(), M, E, c, budget);
	std::vector<unsigned> visits(B * E, 0);
	size_t next = 0;
	auto total = [&](size_t j0, size_t j1, size_t Ec) { return sr_fixed_bytes(nrows0.data(), j0, j1, M, E, c) + sr_s_bytes(j1 - j0, Ec, c.J); };
	for (const SrRound &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= B);
		next = r.j1;
		REQUIRE(r.Ec % 16 == 0 && r.Ec >= 16 && r.Ec <= epad);
		REQUIRE((size_t)r.nchunks * r.Ec >= epad && (size_t)(r.nchunks - 1) * r.Ec < epad);
		REQUIRE(total(r.j0, r.j1, r.Ec) <= budget || (r.j1 - r.j0 == 1 && r.Ec == 16));
		if (r.j1 < B) REQUIRE(total(r.j0, r.j1 + 1, 16) > budget);
		if (r.Ec < epad) REQUIRE(total(r.j0, r.j1, r.Ec + 16) > budget);
		for (unsigned ch = 0; ch < r.nchunks; ch++)
			for (unsigned el = 0; el < r.Ec; el++) {
				const unsigned e = ch * r.Ec + el;
				if (e >= E) continue;
				for (size_t b = r.j0; b < r.j1; b++) visits[b * E + e]++;
			}
		// the table of the round, in a block of its exact size
		const size_t nrows = nrows0[r.j1] - nrows0[r.j0], nt = sr_tiles(nrows0.data(), r.j0, r.j1), nall = (r.j1 - r.j0) * M, nseg = c.segs.size();
		const SrTab t = sr_tab(nseg, epad, nt, nrows, nall);
		const size_t off[6] = {t.segs, t.eps, t.tiles, t.list, t.slot_of, t.bytes};
		const size_t size[5] = {nseg * sizeof(SrSeg), epad * sizeof(double), nt * sizeof(SrTile), nrows * sizeof(unsigned), nall * sizeof(unsigned)};
		const size_t align[5] = {alignof(SrSeg), alignof(double), alignof(SrTile), alignof(unsigned), alignof(unsigned)};
		for (int i = 0; i < 5; i++) REQUIRE(off[i] % align[i] == 0 && off[i] + size[i] <= off[i + 1] && off[i + 1] <= t.bytes);
		std::vector<char> blob(std::max<size_t>(t.bytes, 1), 0);
		blob.shrink_to_fit();
		REQUIRE(sr_fill_round(blob.data(), t, r, M, mtr ? mtr->data() : nullptr, c, eps.data(), E) == nrows);
		const SrSeg *segs = (const SrSeg *)(blob.data() + t.segs);
		const double *ep = (const double *)(blob.data() + t.eps);
		const SrTile *tiles = (const SrTile *)(blob.data() + t.tiles);
		const unsigned *list = (const unsigned *)(blob.data() + t.list), *slot_of = (const unsigned *)(blob.data() + t.slot_of);
		for (size_t s = 0; s < nseg; s++) REQUIRE(segs[s].n0 == c.segs[s].n0 && segs[s].joff == c.segs[s].joff && segs[s].len == c.segs[s].len && segs[s].w == c.segs[s].w);
		for (unsigned e = 0; e < epad; e++) REQUIRE(ep[e] == (e < E ? eps[e] : 0.0));
		size_t ti = 0, slot = 0;
		for (size_t b = r.j0; b < r.j1; b++) {
			std::vector<unsigned> want; // the participating rows of the ensemble, by the rule itself
			for (size_t m = 0; m < M; m++)
				if (!mtr || (*mtr)[b * M + m] > 0) want.push_back((unsigned)m);
			size_t k = 0;
			while (k < want.size()) {
				REQUIRE(ti < nt);
				const SrTile &tl = tiles[ti++];
				REQUIRE(tl.b == b && tl.bl == b - r.j0 && tl.count >= 1 && tl.count <= SR_ROWS && tl.slot0 == slot);
				REQUIRE(tl.count == std::min<size_t>(SR_ROWS, want.size() - k) && tl.slot0 + tl.count <= nrows);
				for (unsigned i = 0; i < tl.count; i++, k++, slot++) {
					REQUIRE(list[tl.slot0 + i] == want[k]);
					REQUIRE(slot_of[(b - r.j0) * M + want[k]] == slot);
				}
			}
			for (size_t m = 0; m < M; m++)
				if (mtr && !((*mtr)[b * M + m] > 0)) REQUIRE(slot_of[(b - r.j0) * M + m] == NOSLOT);
		}
		REQUIRE(ti == nt && slot == nrows);
	}
	REQUIRE(next == B);
	for (unsigned v : visits) REQUIRE(v == 1);
}

int main()
{
	std::mt19937_64 rng(20240611);
	// columns: window edges at and around the multiples of 4 and of the segment length, one to four windows, overlapping or not
	const size_t N = 3 * SR_SEG + 37;
	const size_t edges[] = {0, 1, 3, 4, 5, SR_SEG - 1, SR_SEG, SR_SEG + 1, SR_SEG + 4, 2 * SR_SEG, 2 * SR_SEG + 3, N - 5, N - 1, N};
	const size_t ne = sizeof edges / sizeof *edges;
	for (size_t a = 0; a < ne; a++)
		for (size_t b = a + 1; b < ne; b++) {
			check_columns({edges[a], edges[b]}, N);
			check_columns({edges[a], edges[b], 0, N}, N);
			check_columns({3, 611, edges[a], edges[b], 890, 1501, edges[a], edges[b]}, N);
		}
	// rounds and tables
	const unsigned Es[] = {1, 15, 16, 17, 4096};
	const size_t Bs[] = {1, 2, 3, 7, 40}, Ms[] = {1, 15, 16, 17, 32, 33, 65, 100};
	const std::vector<std::vector<size_t>> wins = {{3, 611}, {3, 611, 890, 1501, 0, 1501}, {0, 1, 5, 6, 0, N, 7, 2 * SR_SEG + 7}};
	unsigned long long nrounds = 0;
	for (const auto &win : wins) {
		const SrCols c = sr_columns(win.data(), (unsigned)(win.size() / 2));
		for (unsigned E : Es) {
			std::vector<double> eps(E);
			for (unsigned e = 0; e < E; e++) eps[e] = -0.4 + 0.8 * (e + 1) / (E + 1);
			for (size_t B : Bs)
				for (size_t M : Ms) {
					if ((size_t)E * B * M > 4096 * 7 * 33) continue; // (keeps the largest tables to a few MB)
					std::vector<unsigned> mtr(B * M);
					for (int pattern = 0; pattern < 3; pattern++) {
						for (size_t i = 0; i < mtr.size(); i++) mtr[i] = pattern == 1 ? (unsigned)(rng() % 3) : 0u; // 1: a third left out; 2: none takes part
						// budgets: tiny (every round one ensemble at 16 stretches), around one ensemble's needs, around the whole call's, huge
						std::vector<size_t> nrows0(B + 1, 0);
						for (size_t b = 0; b < B; b++) nrows0[b + 1] = nrows0[b] + M;
						const size_t one = sr_fixed_bytes(nrows0.data(), 0, 1, M, E, c), all = sr_fixed_bytes(nrows0.data(), 0, B, M, E, c);
						const size_t s16 = sr_s_bytes(1, 16, c.J), sall = sr_s_bytes(B, sr_epad(E), c.J);
						for (size_t budget : {(size_t)1, one + s16 - 1, one + s16, one + 2 * s16, 2 * one + 3 * s16, all + sall / 2, all + sall - 1, all + sall, (size_t)1 << 40}) {
							check_rounds(B, M, E, pattern ? &mtr : nullptr, c, budget, eps);
							nrounds++;
						}
					}
				}
		}
	}
	printf("%llu plans, %llu checks: the columns, rounds and tables agree with the direct enumeration\n", nrounds, nchecks);
	return 0;
}
