// host_plan_check.cpp -- csrc/host_plan.h against a direct enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// host_plan_check` with AddressSanitizer + UBSan; tests/test_host_plan_cpu.py runs it).  It requires:
//   layout      every array of a TableLayout starts aligned for its type, behind the one before, and the block ends with the last
//   rounds      the rounds tile [0, n) in order; a round keeps within the budget unless it is one ensemble; a round that stops early could not
//               have taken the next ensemble
//   slots       participating_rows0 counts, and both slot fillers number, exactly the participating rows in order (h_mtr NULL, all zero and
//               mixed; ens[] all in, all out and mixed): NOSLOT for the others, every callback seen once with its slot, ensemble and row;
//               the arrays are allocated at their exact size, so ASan sees any write past them
//   fitting     largest_fitting returns the largest count that fits, and 1 when none does
//   tasks       the tasks tile the items in order, hold at most `limit` passes unless they are one item, could not have taken the next item,
//               and no task crosses a forced restart; a second call appends behind the tasks of the first
//   ranges      range_error, range_count_error, range_empty_error and range_past_error refuse exactly 0 and more than 4 ranges, n0 >= n1 and
//               n1 > N, each limit from both sides, with the words of the list they are given
#include "host_plan.h"

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

struct Task { unsigned first, n; };

static void check_layout()
{
	struct Wide { double a; unsigned b; };
	TableLayout lay;
	const size_t a = lay.add<char>(3), b = lay.add<double>(2), c = lay.add<unsigned>(0), d = lay.add<Wide>(1), e = lay.add<char>(1), f = lay.add<unsigned>(5);
	REQUIRE(a == 0 && b == 8 && c == 24 && d == 24 && e == 24 + sizeof(Wide) && f == e + 4 && lay.bytes == f + 20);
	REQUIRE(TableLayout().bytes == 0);
}

static void check_rounds(size_t n, const std::vector<size_t> &cost, size_t budget)
{
	auto bytes = [&](size_t j0, size_t j1) { size_t s = 0; for (size_t j = j0; j < j1; j++) s += cost[j]; return s; };
	const std::vector<Round> rounds = whole_ensemble_rounds(n, [&](size_t j0, size_t j1) { return bytes(j0, j1) <= budget; });
	size_t next = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= n);
		next = r.j1;
		REQUIRE(bytes(r.j0, r.j1) <= budget || r.j1 - r.j0 == 1);
		if (r.j1 < n) REQUIRE(bytes(r.j0, r.j1 + 1) > budget);
	}
	REQUIRE(next == n && (n || rounds.empty()));
}

// pattern 0: h_mtr NULL, 1: mixed, 2: all zero
static void check_slots(size_t B, size_t M, int pattern, std::mt19937_64 &rng)
{
	std::vector<unsigned> mtr(B * M);
	for (auto &c : mtr) c = pattern == 2 ? 0 : pattern == 1 ? (unsigned)(rng() % 3) : 5;
	const unsigned *h_mtr = pattern == 0 ? nullptr : mtr.data();
	const std::vector<size_t> nrows0 = participating_rows0(h_mtr, B, M);
	REQUIRE(nrows0.size() == B + 1 && nrows0[0] == 0);
	for (size_t b = 0; b < B; b++) {
		size_t n = 0;
		for (size_t m = 0; m < M; m++) n += mtr[b * M + m] > 0;
		REQUIRE(nrows0[b + 1] == nrows0[b] + n);
	}
	// every round [j0, j1) of the B ensembles
	for (size_t j0 = 0; j0 < B; j0++)
		for (size_t j1 = j0 + 1; j1 <= B; j1++) {
			const size_t nall = (j1 - j0) * M, nrows = nrows0[j1] - nrows0[j0];
			std::vector<unsigned> slot_of(nall, 12345u);
			slot_of.shrink_to_fit();
			std::vector<size_t> seen_b, seen_m;
			const size_t got = fill_round_slots(slot_of.data(), Round{j0, j1}, M, h_mtr, [&](size_t slot, size_t b, size_t m) {
				REQUIRE(slot == seen_b.size());
				seen_b.push_back(b); seen_m.push_back(m);
			});
			REQUIRE(got == nrows && seen_b.size() == nrows);
			size_t slot = 0;
			for (size_t b = j0; b < j1; b++)
				for (size_t m = 0; m < M; m++) {
					const size_t i = (b - j0) * M + m;
					if (mtr[b * M + m] == 0) { REQUIRE(slot_of[i] == NOSLOT); continue; }
					REQUIRE(slot < nrows && slot_of[i] == slot && seen_b[slot] == b && seen_m[slot] == m);
					slot++;
				}
			REQUIRE(slot == nrows);
			// the same rows through ens[]: the ensemble of a participating row, NOSLOT for the others
			std::vector<unsigned> ens(nall), slot_of2(nall, 12345u);
			ens.shrink_to_fit(); slot_of2.shrink_to_fit();
			for (size_t i = 0; i < nall; i++) ens[i] = mtr[j0 * M + i] > 0 ? (unsigned)(j0 + i / M) : NOSLOT;
			REQUIRE(count_slots(ens.data(), nall) == nrows);
			std::vector<size_t> seen_e, seen_i;
			const size_t got2 = fill_row_slots(slot_of2.data(), ens.data(), nall, [&](size_t s, unsigned e, size_t i) {
				REQUIRE(s == seen_e.size());
				seen_e.push_back(e); seen_i.push_back(i);
			});
			REQUIRE(got2 == nrows && seen_e.size() == nrows && slot_of2 == slot_of);
			for (size_t s = 0; s < nrows; s++) REQUIRE(seen_e[s] == seen_b[s] && seen_i[s] == (seen_b[s] - j0) * M + seen_m[s]);
		}
	REQUIRE(count_slots(nullptr, 0) == 0);
}

static void check_fitting()
{
	for (size_t n = 1; n <= 40; n++)
		for (size_t per : {(size_t)1, (size_t)3, (size_t)7})
			for (size_t fixed : {(size_t)0, (size_t)5})
				for (size_t budget = 0; budget <= fixed + per * (n + 1); budget++) {
					auto bytes_of = [&](size_t k) { return fixed + per * k; };
					size_t want = 1;
					for (size_t k = 1; k <= n; k++)
						if (bytes_of(k) <= budget) want = k;
					REQUIRE(largest_fitting(n, bytes_of, budget) == want);
				}
}

// items of 1 .. 4 passes; heads[i] != 0: a run must start at item i
static void check_tasks(const std::vector<unsigned> &passes, const std::vector<char> &heads, unsigned limit, size_t split)
{
	const unsigned n = (unsigned)passes.size();
	std::vector<Task> tasks;
	auto passes_of = [&](unsigned i) { return passes[i]; };
	auto restart = [&](unsigned i) { return heads[i] != 0; };
	// in one call, or in two that meet at `split` (a head: the second call appends behind the tasks of the first)
	if (split < n && heads[split]) {
		pack_tasks(tasks, 0, (unsigned)split, limit, passes_of, restart);
		pack_tasks(tasks, (unsigned)split, n, limit, passes_of, restart);
	} else
		pack_tasks(tasks, 0, n, limit, passes_of, restart);
	unsigned next = 0;
	for (size_t t = 0; t < tasks.size(); t++) {
		const Task &k = tasks[t];
		REQUIRE(k.first == next && k.n >= 1 && k.first + k.n <= n);
		next = k.first + k.n;
		unsigned sum = 0;
		for (unsigned i = k.first; i < next; i++) {
			sum += passes[i];
			if (i > k.first) REQUIRE(!heads[i]); // no run crosses a forced restart
		}
		REQUIRE(sum <= limit || k.n == 1);
		if (next < n && !heads[next]) REQUIRE(sum + passes[next] > limit); // maximal
	}
	REQUIRE(next == n && (n || tasks.empty()));
}

static void check_ranges()
{
	for (const RangeWords *what : {&WINDOWS, &LAG_RANGES}) {
		const size_t five[10] = {0, 9, 0, 9, 0, 9, 0, 9, 0, 9};
		REQUIRE(range_error(five, 0, *what) == what->count && !range_error(five, 1, *what) && !range_error(five, 4, *what) && range_error(five, 5, *what) == what->count);
		REQUIRE(range_error(five, ~0u, *what) == what->count && range_count_error(0, *what) && !range_count_error(1, *what) && !range_count_error(4, *what) &&
		        range_count_error(5, *what));
		const size_t one[2] = {5, 6}, empty[2] = {6, 6}, back[2] = {7, 6};
		REQUIRE(!range_error(one, 1, *what) && range_error(empty, 1, *what) == what->empty && range_error(back, 1, *what) == what->empty);
		const size_t mixed[8] = {0, 9, 4, 4, 0, 9, 0, 9};
		REQUIRE(range_error(mixed, 4, *what) == what->empty && !range_error(mixed, 1, *what) && !range_error(mixed + 4, 2, *what));
		REQUIRE(range_error(mixed, 5, *what) == what->count); // (the count first: nothing past the list's end is read)
		REQUIRE(!range_empty_error(mixed, 0, *what) && !range_empty_error(mixed, 1, *what) && range_empty_error(mixed, 2, *what) == what->empty);
		REQUIRE(range_empty_error(five, 5, *what) == nullptr); // (a list of B W ranges may be longer than 4)
		REQUIRE(!range_past_error(five, 5, 9, *what) && !range_past_error(five, 5, 10, *what) && range_past_error(five, 5, 8, *what) == what->past);
		const size_t last[4] = {0, 9, 3, 10};
		REQUIRE(range_past_error(last, 2, 9, *what) == what->past && !range_past_error(last, 1, 9, *what) && !range_past_error(last, 2, 10, *what) &&
		        !range_past_error(last, 0, 0, *what));
	}
	REQUIRE(!strcmp(WINDOWS.count, "1 to 4 windows") && !strcmp(WINDOWS.empty, "an empty window (n0 >= n1)") && !strcmp(WINDOWS.past, "a window past the trace length"));
	REQUIRE(!strcmp(LAG_RANGES.count, "1 to 4 lag ranges") && !strcmp(LAG_RANGES.empty, "an empty lag range (n0 >= n1)") &&
	        !strcmp(LAG_RANGES.past, "a lag range past the trace length"));
}

int main()
{
	std::mt19937_64 rng(20241203);
	unsigned long long nrounds = 0, nslots = 0, ntasks = 0;
	check_layout();
	check_ranges();
	check_fitting();
	for (size_t n = 0; n <= 5; n++)
		for (int rep = 0; rep < 20; rep++) {
			std::vector<size_t> cost(n);
			size_t all = 0, top = 0;
			for (auto &c : cost) { c = rep ? (size_t)(rng() % 9) : 4; all += c; top = std::max(top, c); }
			for (size_t budget : {(size_t)0, (size_t)1, top - (top > 0), top, top + 1, 2 * top, all - (all > 0), all, all + 1, (size_t)1 << 40}) {
				check_rounds(n, cost, budget);
				nrounds++;
			}
		}
	for (size_t B = 1; B <= 5; B++)
		for (size_t M = 1; M <= 4; M++)
			for (int pattern = 0; pattern < 3; pattern++)
				for (int rep = 0; rep < (pattern == 1 ? 8 : 1); rep++) { check_slots(B, M, pattern, rng); nslots++; }
	REQUIRE(participating_rows0(nullptr, 0, 3) == std::vector<size_t>(1, 0));
	for (unsigned n = 0; n <= 40; n++)
		for (int rep = 0; rep < 12; rep++) {
			std::vector<unsigned> passes(n);
			std::vector<char> heads(n);
			for (auto &p : passes) p = rep == 0 ? 4 : rep == 1 ? 1 : 1 + (unsigned)(rng() % 4);
			for (auto &h : heads) h = rep % 3 == 2 ? rng() % 5 == 0 : 0;
			for (unsigned limit : {4u, 5u, 16u})
				for (size_t split : {(size_t)n, (size_t)(n / 2), (size_t)(n / 3)}) {
					if (split < n) heads[split] = 1;
					check_tasks(passes, heads, limit, split);
					ntasks++;
				}
		}
	printf("%llu round plans, %llu participation patterns, %llu task lists, %llu checks: the layout, rounds, slots, fitting, tasks and ranges agree with the direct enumeration\n",
	       nrounds, nslots, ntasks, nchecks);
	return 0;
}
