// dtw_plan_check.cpp -- csrc/dtw_plan.h against a direct enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// dtw_plan_check` with AddressSanitizer + UBSan; tests/test_dtw_plan_cpu.py runs it).  It requires:
//   parameters  dt_par_error refuses exactly Lmax outside [1, 127] and b outside [1, 8], dt_range_error exactly W outside [1, 4], n0 >= n1 and
//               ranges longer than 131072, each limit from both sides
//   geometry    nl = 2 Lmax + 1; Q the smallest of 1, 2, 4 with 64 Q >= nl, and 64 Q > nl; sample by sample, the lag offsets and T; sample by
//               sample, the word and bit position of every choice lies inside the range's plane and no two samples share one; the planes of
//               the ranges tile the row's P words; a range alone has the same sizes
//   LDS         the rings, the two staged chunks and the backtrack block lie inside the wave's bytes, the forward arrays disjoint, below 64 KiB
//   rounds      the rounds tile the ensembles in order; planes and table stay within the budget unless the round is one ensemble; a round that
//               stops early could not have taken the next ensemble
//   table       the block (allocated at its exact size: ASan sees any write past it) holds the slot of every row, numbering the participating
//               rows of the round in order, NOSLOT for the others
#include "dtw_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

static unsigned long long nchecks = 0;
#define REQUIRE(c)                                                                 \
	do {                                                                           \
		nchecks++;                                                                 \
		if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
	} while (0)

static void check_params()
{
	for (unsigned L = 0; L < 300; L++)
		for (unsigned b = 0; b < 12; b++) REQUIRE((dt_par_error({L, b}) == nullptr) == (L >= 1 && L <= 127 && b >= 1 && b <= 8));
	REQUIRE(dt_par_error({0, 1}) && !dt_par_error({1, 1}) && !dt_par_error({127, 8}) && dt_par_error({128, 8}) && dt_par_error({127, 9}) && dt_par_error({127, 0}));
	REQUIRE(dt_par_error({~0u, 1}) && dt_par_error({1, ~0u}));
	const size_t one[2] = {5, 6}, empty[2] = {6, 6}, back[2] = {7, 6}, longest[2] = {3, 3 + 131072}, too_long[2] = {3, 3 + 131073};
	REQUIRE(!dt_range_error(one, 1) && dt_range_error(empty, 1) && dt_range_error(back, 1) && !dt_range_error(longest, 1) && dt_range_error(too_long, 1));
	const size_t five[10] = {0, 9, 0, 9, 0, 9, 0, 9, 0, 9};
	REQUIRE(dt_range_error(five, 0) && !dt_range_error(five, 1) && !dt_range_error(five, 4) && dt_range_error(five, 5));
	const size_t mixed[8] = {0, 9, 4, 4, 0, 9, 0, 9}, mixed2[8] = {0, 9, 0, 9, 0, 9, 0, 200000};
	REQUIRE(dt_range_error(mixed, 4) && !dt_range_error(mixed, 1) && dt_range_error(mixed2, 4) && !dt_range_error(mixed2, 3));
}

static void check_geom(const DtwPar &p, const std::vector<size_t> &win)
{
	const unsigned W = (unsigned)(win.size() / 2);
	REQUIRE(!dt_par_error(p) && !dt_range_error(win.data(), W));
	const DtwGeom g = dt_geom(p, win.data(), W);
	REQUIRE(g.nl == 2 * p.Lmax + 1 && (g.Q == 1 || g.Q == 2 || g.Q == 4) && g.nlp == 64 * g.Q && g.nlp > g.nl && (g.Q == 1 || 32 * g.Q < g.nl) && g.W == W);
	size_t t = 0;
	unsigned long long pw = 0;
	for (unsigned w = 0; w < W; w++) {
		REQUIRE(g.off[w] == t && g.poff[w] == pw && g.n0[w] == win[2 * w]);
		std::set<unsigned long long> used;
		unsigned top = 0;
		for (size_t n = win[2 * w]; n < win[2 * w + 1]; n++, t++) {
			const unsigned i = (unsigned)(n - win[2 * w]), word = i / 16, bit = 2 * (i % 16);
			REQUIRE(word < g.words[w] && bit < 32 && used.insert((unsigned long long)word * 32 + bit).second);
			top = std::max(top, word);
		}
		REQUIRE(g.n[w] == win[2 * w + 1] - win[2 * w] && top + 1 == g.words[w]); // (no word without a sample)
		pw += (unsigned long long)g.words[w] * g.nlp;
		const DtwGeom one = dt_geom(p, &win[2 * w], 1);
		REQUIRE(one.n[0] == g.n[w] && one.words[0] == g.words[w] && one.T() == g.n[w] && one.P() == (unsigned long long)g.words[w] * g.nlp && one.n0[0] == g.n0[w]);
	}
	for (unsigned w = W; w <= DT_WMAX; w++) REQUIRE(g.off[w] == t && g.poff[w] == pw);
	for (unsigned w = W; w < DT_WMAX; w++) REQUIRE(g.n[w] == 0 && g.words[w] == 0);
	REQUIRE(g.T() == t && g.P() == pw);

	const DtwLds l = dt_lds(p, g.Q);
	const unsigned ring = p.b > 1 ? 64 * g.Q * 8 : 0;
	REQUIRE(l.ringD == 0 && l.ringE == p.b * ring && l.stage == l.ringE + (p.b - 1) * ring && l.stage % 16 == 0);
	REQUIRE(l.stage_doubles == 64 + 64 + 64 * g.Q && l.stage_doubles >= 64 + 64 + 2 * p.Lmax); // a chunk's row samples and its reach of the reference
	REQUIRE(l.stage + 2 * l.stage_doubles * 8 <= l.bytes);
	REQUIRE(l.back_words == 0 && l.back_lags == DT_BACK * g.nlp * 4 && l.back_lags + 16 * DT_BACK * 4 <= l.bytes && l.bytes <= 65536);
}

static void check_rounds(const DtwPar &p, const std::vector<size_t> &win, size_t B, size_t M, int pattern, size_t budget, std::mt19937_64 &rng)
{
	const DtwGeom g = dt_geom(p, win.data(), (unsigned)(win.size() / 2));
	std::vector<unsigned> mtr(B * M);
	for (auto &c : mtr) c = pattern == 2 ? 0 : pattern == 1 ? (unsigned)(rng() % 3) : 5;
	std::vector<size_t> nrows0(B + 1, 0);
	for (size_t e = 0; e < B; e++) {
		size_t n = 0;
		for (size_t m = 0; m < M; m++) n += mtr[e * M + m] > 0;
		nrows0[e + 1] = nrows0[e] + n;
	}
	const std::vector<Round> rounds = dt_rounds(B, nrows0.data(), M, g, budget);
	size_t next = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= B);
		next = r.j1;
		const size_t nb = r.j1 - r.j0, nrows = nrows0[r.j1] - nrows0[r.j0];
		size_t words = 0;
		for (size_t i = 0; i + 1 < win.size(); i += 2) words += (win[i + 1] - win[i] + 15) / 16 * g.nlp;
		REQUIRE(dt_round_bytes(nrows0.data(), r.j0, r.j1, M, g) == nrows * words * 4 + nb * M * 4);
		REQUIRE(dt_round_bytes(nrows0.data(), r.j0, r.j1, M, g) <= budget || nb == 1);
		if (r.j1 < B) REQUIRE(dt_round_bytes(nrows0.data(), r.j0, r.j1 + 1, M, g) > budget);
		const DtwTab t = dt_tab(nb * M);
		REQUIRE(t.slot_of == 0 && t.bytes == nb * M * 4);
		std::vector<char> blob(std::max<size_t>(t.bytes, 1), 0);
		blob.shrink_to_fit();
		REQUIRE(dt_fill_round(blob.data(), t, r, M, pattern == 0 ? nullptr : mtr.data()) == nrows);
		const unsigned *slot_of = (const unsigned *)(blob.data() + t.slot_of);
		size_t slot = 0;
		for (size_t e = r.j0; e < r.j1; e++)
			for (size_t m = 0; m < M; m++) {
				const size_t i = (e - r.j0) * M + m;
				if (mtr[e * M + m] == 0) { REQUIRE(slot_of[i] == NOSLOT); continue; }
				REQUIRE(slot < nrows && slot_of[i] == slot);
				slot++;
			}
		REQUIRE(slot == nrows);
	}
	REQUIRE(next == B);
}

int main()
{
	std::mt19937_64 rng(20241120);
	unsigned long long ngeom = 0, nrounds = 0;
	check_params();
	const size_t N = 1501;
	const unsigned Ls[] = {1, 31, 32, 127}, bs[] = {1, 8};
	const size_t e[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 611, 700, 701, N - 17, N - 16, N - 1, N};
	const size_t ne = sizeof e / sizeof *e;
	const std::vector<size_t> win = {0, N, 700, 701, 650, 652, 100, 700};
	for (unsigned L : Ls)
		for (unsigned b : bs) {
			const DtwPar p = {L, b};
			for (size_t a = 0; a < ne; a++)
				for (size_t c = a + 1; c < ne; c++) { check_geom(p, {e[a], e[c]}); ngeom++; }
			check_geom(p, win);
			check_geom(p, {3, 611, 3, 611, 0, 16});
			check_geom(p, {0, 131072});
			ngeom += 3;
			for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)40})
				for (size_t M : {(size_t)1, (size_t)9, (size_t)33}) {
					std::vector<size_t> full(B + 1);
					for (size_t i = 0; i <= B; i++) full[i] = i * M;
					const DtwGeom g = dt_geom(p, win.data(), 4);
					const size_t one = dt_round_bytes(full.data(), 0, 1, M, g), all = dt_round_bytes(full.data(), 0, B, M, g);
					for (int pattern = 0; pattern < 3; pattern++)
						for (size_t budget : {(size_t)1, one - 1, one, one + 1, 2 * one, 2 * one + one / 2, all - 1, all, (size_t)1 << 40}) {
							check_rounds(p, win, B, M, pattern, budget, rng);
							nrounds++;
						}
				}
		}
	printf("%llu range sets, %llu round plans, %llu checks: the parameters, samples, offsets, planes, LDS, rounds and tables agree with the direct enumeration\n",
	       ngeom, nrounds, nchecks);
	return 0;
}
