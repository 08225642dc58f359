// filter_plan_check.cpp -- csrc/filter_plan.h against a direct enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// filter_plan_check` with AddressSanitizer + UBSan; tests/test_filter_traces_cpu.py runs it).  It requires:
//   slabs    every participating row of a pass lies in exactly one slab, no row left out in any; a slab holds 1 .. CF_SLAB consecutive rows of
//            ONE ensemble; the slabs are in row order; and none could have taken the next row (it is left out, of another ensemble, not
//            adjacent, or the slab is full)
//   rounds   the rounds tile the ensembles in order; a round's blocks stay within the budget unless it is one ensemble (cf_round_fits tells);
//            a round that stops early could not have taken the next ensemble; no round holds more than CF_MAX_ENS ensembles
//   chunks   a chunk of rows of one ensemble fits or is one row, and one more row would not fit; the rows of one inverse call are all of them
//            or an even number that fits (two at least), and two more would not
//   table    every array of the block lies inside it, aligned, none overlapping (the block is allocated at its exact size: ASan sees any
//            write past it); the slabs, the ensembles and the rows' flags read back as written
#include "filter_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static unsigned long long nchecks = 0;
#define REQUIRE(c)                                                                 \
	do {                                                                           \
		nchecks++;                                                                 \
		if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
	} while (0)

static void check_slabs(const std::vector<unsigned> &ens)
{
	const size_t n = ens.size();
	const std::vector<CfSlab> slabs = cf_slabs(ens.data(), n);
	std::vector<int> seen(n, 0);
	size_t next = 0;
	for (size_t k = 0; k < slabs.size(); k++) {
		const CfSlab &s = slabs[k];
		REQUIRE(s.n >= 1 && s.n <= CF_SLAB && (size_t)s.row0 + s.n <= n && s.row0 >= next);
		for (unsigned r = 0; r < s.n; r++) {
			REQUIRE(ens[s.row0 + r] == s.ens && s.ens != NOSLOT);
			seen[s.row0 + r]++;
		}
		for (size_t i = next; i < s.row0; i++) REQUIRE(ens[i] == NOSLOT); // only rows left out lie between two slabs
		next = (size_t)s.row0 + s.n;
		// maximal: the next row could not have joined
		if (next < n && s.n < CF_SLAB) REQUIRE(ens[next] != s.ens);
	}
	for (size_t i = next; i < n; i++) REQUIRE(ens[i] == NOSLOT);
	for (size_t i = 0; i < n; i++) REQUIRE(seen[i] == (ens[i] != NOSLOT));

	// the table block, at its exact size
	std::vector<CfEns> en;
	unsigned nens = 0;
	for (unsigned e : ens) if (e != NOSLOT) nens = std::max(nens, e + 1);
	for (unsigned e = 0; e < nens; e++) en.push_back({(double)(e + 2), (int)(e % 4), 0u});
	const CfTab o = cf_tab(slabs.size(), nens, n);
	REQUIRE(o.ens % alignof(CfEns) == 0 && o.slabs % alignof(CfSlab) == 0 && o.live % alignof(unsigned) == 0);
	REQUIRE(o.ens + nens * sizeof(CfEns) <= o.slabs && o.slabs + slabs.size() * sizeof(CfSlab) <= o.live && o.live + n * sizeof(unsigned) == o.bytes);
	char *blob = (char *)malloc(o.bytes ? o.bytes : 1);
	cf_fill(blob, o, slabs, en.data(), nens, ens.data(), n);
	for (unsigned e = 0; e < nens; e++) {
		CfEns x;
		memcpy(&x, blob + o.ens + e * sizeof(CfEns), sizeof x);
		REQUIRE(x.K == en[e].K && x.mode == en[e].mode);
	}
	for (size_t k = 0; k < slabs.size(); k++) {
		CfSlab x;
		memcpy(&x, blob + o.slabs + k * sizeof(CfSlab), sizeof x);
		REQUIRE(x.row0 == slabs[k].row0 && x.n == slabs[k].n && x.ens == slabs[k].ens);
	}
	for (size_t i = 0; i < n; i++) {
		unsigned x;
		memcpy(&x, blob + o.live + i * sizeof(unsigned), sizeof x);
		REQUIRE(x == (ens[i] != NOSLOT));
	}
	free(blob);
	// an upper bound of the lengths gives an upper bound of the block
	REQUIRE(cf_tab(n, nens + 3, n + 5).bytes >= o.bytes);
}

static void check_rounds(const std::vector<size_t> &rows0, const CfCost &c, size_t budget)
{
	const size_t B = rows0.size() - 1;
	const std::vector<Round> rounds = cf_rounds(rows0.data(), B, c, budget);
	size_t at = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == at && r.j1 > r.j0 && r.j1 <= B && r.j1 - r.j0 <= CF_MAX_ENS);
		const size_t bytes = c.fixed + (r.j1 - r.j0) * c.ens_bytes + (rows0[r.j1] - rows0[r.j0]) * c.row_bytes;
		REQUIRE(cf_round_fits(rows0.data(), r, c, budget) == (bytes <= budget));
		REQUIRE(bytes <= budget || r.j1 - r.j0 == 1);
		if (r.j1 < B && r.j1 - r.j0 < CF_MAX_ENS)
			REQUIRE(c.fixed + (r.j1 + 1 - r.j0) * c.ens_bytes + (rows0[r.j1 + 1] - rows0[r.j0]) * c.row_bytes > budget);
		if (bytes > budget && rows0[r.j1] > rows0[r.j0]) { // worked in chunks (an ensemble without target rows has no work)
			const size_t n = rows0[r.j1] - rows0[r.j0], k = cf_chunk_rows(n, c, budget);
			REQUIRE(k >= 1 && k <= n);
			REQUIRE(k == 1 || cf_bytes(c, 1, k) <= budget);
			REQUIRE(k == n || cf_bytes(c, 1, k + 1) > budget);
		}
		at = r.j1;
	}
	REQUIRE(at == B);
}

int main()
{
	std::mt19937_64 rng(20240607);
	// slabs: hand cases, then random passes
	check_slabs({});
	check_slabs({NOSLOT, NOSLOT});
	check_slabs({0, 0, 0, 0, 0, 0, 0, 0});
	check_slabs({0, 0, 0, 0, 0, 0, 0, 0, 0});
	check_slabs({0, 1, 1, NOSLOT, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, NOSLOT});
	for (int t = 0; t < 400; t++) {
		const size_t n = 1 + rng() % 200;
		std::vector<unsigned> ens(n);
		unsigned e = 0;
		for (size_t i = 0; i < n; i++) {
			if (rng() % 11 == 0) e++;
			ens[i] = rng() % 9 == 0 ? NOSLOT : e;
		}
		check_slabs(ens);
	}
	// rounds and chunks: frames of several sizes, budgets from one row to everything
	for (int t = 0; t < 400; t++) {
		const size_t ncoef = 100 + rng() % 9000, N = 64 + rng() % 4000, inv = std::max<size_t>(ncoef * 16, (1 + rng() % 12) * N * 8);
		const unsigned Kmax = (unsigned)(rng() % 3 ? 0 : 4);
		const CfCost c = cf_cost(ncoef, N, Kmax);
		REQUIRE(c.row_bytes == ncoef * 16 + N * 8 && c.ens_bytes == ncoef * 24 && c.fixed == ncoef * 16 + Kmax * N * 8);
		for (size_t n : {(size_t)1, (size_t)2, (size_t)7, (size_t)500})
			for (size_t budget : {(size_t)1, inv, 2 * inv, 9 * inv + 5, 1000 * inv}) {
				const size_t k = cf_inverse_rows(n, inv, budget);
				REQUIRE(k >= 1 && k <= n && (k == n || (k % 2 == 0 && (k == 2 || k * inv <= budget) && (k + 2) * inv > budget)));
			}
		const size_t B = 1 + rng() % 12;
		std::vector<size_t> rows0(B + 1, 0);
		for (size_t b = 0; b < B; b++) rows0[b + 1] = rows0[b] + (rng() % 5 == 0 ? 0 : rng() % 90);
		const size_t all = cf_bytes(c, B, rows0[B]);
		for (size_t budget : {(size_t)1, c.row_bytes, cf_bytes(c, 1, 1), cf_bytes(c, 1, 7), all / 3, all - 1, all, all * 2}) check_rounds(rows0, c, budget);
	}
	printf("filter_plan_check: %llu checks agree with the direct enumeration\n", nchecks);
	return 0;
}
