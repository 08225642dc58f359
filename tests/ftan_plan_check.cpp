// ftan_plan_check.cpp -- csrc/ftan_plan.h against a direct per-index enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// ftan_plan_check` with AddressSanitizer + UBSan; tests/test_ftan_plan_cpu.py runs it).  It requires:
//   classes  two ensembles share a class iff their window sets (and noise ranges, when noise is wanted) are equal by value; the classes are
//            numbered in order of first appearance and first_of names the first ensemble of each
//   items    for every (class, scale of the range, window) the indices k with n0 <= k D < n1 -- and, under the wrap rule, with their filter
//            support [k D - c, k D - c + L) inside [0, N), decided per index -- are exactly the ones the span's items hold, each once; the
//            items of a span start at the range's first member plus multiples of FT_SEG, hold 1 .. FT_SEG members, carry the scale's offset
//            and length and the kind; likewise for (class, scale, noise range); the class brackets exactly its items, peak items first; the
//            plan of one ensemble, one window and one scale alone gives the same items
//   tasks    the tasks of a class tile its items in order, each of at most FT_TASK passes, none across two classes, and no task could have
//            taken the next item of its class; max_items and max_tasks are the largest class's
//   rounds   the rounds tile the ensembles in order; sets, partial results and table stay within the budget unless the round is one ensemble;
//            a round that stops early could not have taken the next ensemble; a chunk of rows fits or is one row, and one more would not fit
//   table    every array of the block lies inside it, aligned, none overlapping (the block is allocated at its exact size: ASan sees any
//            write past it); the list holds each participating row once, in order, with its ensemble's class; slot_of inverts it
#include "ftan_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

static unsigned long long nchecks = 0;
#define REQUIRE(c)                                                                 \
	do {                                                                           \
		nchecks++;                                                                 \
		if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
	} while (0)

struct Frame { std::vector<WxScale> sc; size_t N, ncoef; };

// a frame in the library's shape: J octaves of V voices, D = 2^(octave + 1) (or odd decimations when `odd`), Ns = ceil(N / D), filters that
// grow with the scale and may be longer than the trace
static Frame make_frame(size_t N, unsigned J, unsigned V, bool odd, std::mt19937_64 &rng)
{
	Frame f;
	f.N = N;
	unsigned long long off = 0;
	for (unsigned j = 0; j < J; j++)
		for (unsigned v = 0; v < V; v++) {
			WxScale s;
			s.D = odd ? 2 * j + 3 : 2u << j;
			s.Ns = (unsigned)((N + s.D - 1) / s.D);
			s.L = (unsigned)((8u << j) + 3 * v + rng() % 5);
			s.c = (int)(s.L / 2) - (int)(rng() % 3) + (j == 0 && v == 0 ? -(int)(s.L / 2) - 1 : 0); // (one scale with a negative centre)
			s.coef_off = off;
			s.omega = 0.0;
			off += s.Ns;
			f.sc.push_back(s);
		}
	f.ncoef = (size_t)off;
	return f;
}

static bool takes_part(const WxScale &s, size_t N, size_t k, size_t n0, size_t n1, int skip)
{
	const long long at = (long long)k * s.D;
	if (at < (long long)n0 || at >= (long long)n1) return false;
	if (!skip) return true;
	const long long a = at - s.c, b = a + s.L; // the filter support [a, b)
	return a >= 0 && b <= (long long)N;
}

static bool same_item(const FtItem &a, const FtItem &b) { return a.base == b.base && a.k0 == b.k0 && a.count == b.count && a.Ns == b.Ns && a.noise == b.noise; }

// the items of one span against the enumeration of [n0, n1)
static void check_span(const Frame &f, const FtPlan &p, const FtSpan sp, const WxScale &s, size_t n0, size_t n1, int skip, unsigned kind)
{
	std::vector<unsigned char> seen(s.Ns, 0);
	size_t first = s.Ns;
	for (size_t k = 0; k < s.Ns; k++)
		if (takes_part(s, f.N, k, n0, n1, skip)) { first = k; break; }
	for (unsigned i = 0; i < sp.n; i++) {
		REQUIRE(sp.first + i < p.items.size());
		const FtItem &it = p.items[sp.first + i];
		REQUIRE(it.count >= 1 && it.count <= FT_SEG && it.k0 == first + (size_t)i * FT_SEG && it.base == s.coef_off && it.Ns == s.Ns && it.noise == kind);
		REQUIRE((size_t)it.k0 + it.count <= s.Ns && it.base + it.Ns <= f.ncoef);
		REQUIRE(i + 1 == sp.n || it.count == FT_SEG);
		for (unsigned j = 0; j < it.count; j++) { REQUIRE(!seen[it.k0 + j]); seen[it.k0 + j] = 1; }
	}
	for (size_t k = 0; k < s.Ns; k++) REQUIRE(seen[k] == takes_part(s, f.N, k, n0, n1, skip));
}

static void check_plan(const Frame &f, unsigned s0, unsigned s1, const std::vector<size_t> &win, unsigned W, const std::vector<size_t> &noise, size_t B, int skip)
{
	const unsigned S = (unsigned)f.sc.size(), Sx = s1 - s0;
	const size_t *nz = noise.empty() ? nullptr : noise.data();
	const FtPlan p = ft_plan(f.sc.data(), S, f.N, s0, s1, win.data(), W, nz, B, skip);
	REQUIRE(p.W == W && p.Sx == Sx && p.noise == (nz != nullptr) && p.cls_of.size() == B && p.scales.size() == Sx);
	for (unsigned sx = 0; sx < Sx; sx++) REQUIRE(p.scales[sx].base == f.sc[s0 + sx].coef_off && p.scales[sx].D == f.sc[s0 + sx].D && p.scales[sx].Ns == f.sc[s0 + sx].Ns);
	// classes: equality by value, numbered by first appearance
	auto equal = [&](size_t a, size_t b) {
		for (unsigned i = 0; i < 2 * W; i++)
			if (win[a * 2 * W + i] != win[b * 2 * W + i]) return false;
		return !nz || (nz[2 * a] == nz[2 * b] && nz[2 * a + 1] == nz[2 * b + 1]);
	};
	unsigned ncls = 0;
	for (size_t b = 0; b < B; b++) {
		size_t a = 0;
		while (a < b && !equal(a, b)) a++;
		if (a == b) { REQUIRE(p.cls_of[b] == ncls && ncls < p.first_of.size() && p.first_of[ncls] == b); ncls++; }
		else REQUIRE(p.cls_of[b] == p.cls_of[a]);
	}
	REQUIRE(ncls == p.first_of.size() && ncls == p.classes.size() && p.pspans.size() == (size_t)ncls * Sx * W && p.nspans.size() == (nz ? (size_t)ncls * Sx : 0));
	unsigned next = 0, next_task = 0, max_items = 0, max_tasks = 0;
	for (unsigned c = 0; c < ncls; c++) {
		const size_t b = p.first_of[c];
		const FtClass &cl = p.classes[c];
		REQUIRE(cl.item0 == next && cl.task0 == next_task);
		for (unsigned sx = 0; sx < Sx; sx++)
			for (unsigned w = 0; w < W; w++) {
				const FtSpan sp = p.pspans[((size_t)c * Sx + sx) * W + w];
				REQUIRE(sp.first == next);
				next += sp.n;
				check_span(f, p, sp, f.sc[s0 + sx], win[(b * W + w) * 2], win[(b * W + w) * 2 + 1], skip, 0);
				// the same items from this ensemble, this window and this scale alone
				const FtPlan q = ft_plan(f.sc.data(), S, f.N, s0 + sx, s0 + sx + 1, &win[(b * W + w) * 2], 1, nullptr, 1, skip);
				REQUIRE(q.classes.size() == 1 && q.pspans.size() == 1 && q.pspans[0].n == sp.n && q.items.size() == sp.n);
				for (unsigned i = 0; i < sp.n; i++) REQUIRE(same_item(q.items[i], p.items[sp.first + i]));
			}
		for (unsigned sx = 0; nz && sx < Sx; sx++) {
			const FtSpan sp = p.nspans[(size_t)c * Sx + sx];
			REQUIRE(sp.first == next);
			next += sp.n;
			check_span(f, p, sp, f.sc[s0 + sx], nz[2 * b], nz[2 * b + 1], skip, 1);
		}
		REQUIRE(cl.nitems == next - cl.item0);
		// the tasks of the class
		unsigned at = cl.item0;
		for (unsigned t = 0; t < cl.ntasks; t++) {
			REQUIRE(cl.task0 + t < p.tasks.size());
			const FtTask &tk = p.tasks[cl.task0 + t];
			REQUIRE(tk.first == at && tk.n >= 1 && tk.first + tk.n <= cl.item0 + cl.nitems);
			unsigned passes = 0;
			for (unsigned i = 0; i < tk.n; i++) passes += (p.items[tk.first + i].count + 63) / 64;
			REQUIRE(passes <= FT_TASK);
			at += tk.n;
			if (at < cl.item0 + cl.nitems) REQUIRE(passes + (p.items[at].count + 63) / 64 > FT_TASK);
		}
		REQUIRE(at == cl.item0 + cl.nitems && (cl.ntasks > 0) == (cl.nitems > 0));
		next_task += cl.ntasks;
		max_items = std::max(max_items, cl.nitems);
		max_tasks = std::max(max_tasks, cl.ntasks);
	}
	REQUIRE(next == p.items.size() && next_task == p.tasks.size() && max_items == p.max_items && max_tasks == p.max_tasks);
}

static void check_rounds(const Frame &f, const FtPlan &p, size_t B, size_t M, unsigned P, int pattern, size_t budget, std::mt19937_64 &rng)
{
	auto total = [&](size_t nb) { return ft_set_bytes(nb, M, f.ncoef) + ft_pass_bytes(p, P, nb * M); };
	const std::vector<Round> rounds = ft_rounds(B, M, f.ncoef, p, P, budget);
	size_t next = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= B);
		next = r.j1;
		REQUIRE(total(r.j1 - r.j0) <= budget || r.j1 - r.j0 == 1);
		if (r.j1 < B) REQUIRE(total(r.j1 + 1 - r.j0) > budget);
		// the table of the round, in a block of its exact size
		const size_t nrows = (r.j1 - r.j0) * M;
		std::vector<unsigned> ens(nrows);
		for (size_t i = 0; i < nrows; i++) ens[i] = pattern == 2 || (pattern == 1 && rng() % 3 == 0) ? NOSLOT : (unsigned)(r.j0 + i / M);
		const size_t nslots = count_slots(ens.data(), nrows);
		const FtTab t = ft_tab(p, nslots, nrows);
		const size_t off[9] = {t.items, t.tasks, t.classes, t.pspans, t.nspans, t.scales, t.list, t.slot_of, t.bytes};
		const size_t size[8] = {p.items.size() * sizeof(FtItem), p.tasks.size() * sizeof(FtTask), p.classes.size() * sizeof(FtClass), p.pspans.size() * sizeof(FtSpan),
		                        p.nspans.size() * sizeof(FtSpan), p.scales.size() * sizeof(FtScale), nslots * sizeof(FtRow), nrows * sizeof(unsigned)};
		const size_t align[8] = {alignof(FtItem), alignof(FtTask), alignof(FtClass), alignof(FtSpan), alignof(FtSpan), alignof(FtScale), alignof(FtRow), alignof(unsigned)};
		for (int i = 0; i < 8; i++) REQUIRE(off[i] % align[i] == 0 && off[i] + size[i] <= off[i + 1] && off[i + 1] <= t.bytes);
		REQUIRE(t.bytes <= ft_tab(p, nrows, nrows).bytes && ft_part_bytes(p, P, nslots) + t.bytes <= ft_pass_bytes(p, P, nrows));
		std::vector<char> blob(std::max<size_t>(t.bytes, 1), 0);
		blob.shrink_to_fit();
		REQUIRE(ft_fill(blob.data(), t, p, ens.data(), nrows) == nslots);
		const FtItem *items = (const FtItem *)(blob.data() + t.items);
		const FtTask *tasks = (const FtTask *)(blob.data() + t.tasks);
		const FtClass *classes = (const FtClass *)(blob.data() + t.classes);
		const FtSpan *pspans = (const FtSpan *)(blob.data() + t.pspans), *nspans = (const FtSpan *)(blob.data() + t.nspans);
		const FtScale *scales = (const FtScale *)(blob.data() + t.scales);
		const FtRow *list = (const FtRow *)(blob.data() + t.list);
		const unsigned *slot_of = (const unsigned *)(blob.data() + t.slot_of);
		for (size_t i = 0; i < p.items.size(); i++) REQUIRE(same_item(items[i], p.items[i]));
		for (size_t i = 0; i < p.tasks.size(); i++) REQUIRE(tasks[i].first == p.tasks[i].first && tasks[i].n == p.tasks[i].n);
		for (size_t i = 0; i < p.classes.size(); i++)
			REQUIRE(classes[i].item0 == p.classes[i].item0 && classes[i].nitems == p.classes[i].nitems && classes[i].task0 == p.classes[i].task0 && classes[i].ntasks == p.classes[i].ntasks);
		for (size_t i = 0; i < p.pspans.size(); i++) REQUIRE(pspans[i].first == p.pspans[i].first && pspans[i].n == p.pspans[i].n);
		for (size_t i = 0; i < p.nspans.size(); i++) REQUIRE(nspans[i].first == p.nspans[i].first && nspans[i].n == p.nspans[i].n);
		for (size_t i = 0; i < p.scales.size(); i++) REQUIRE(scales[i].base == p.scales[i].base && scales[i].D == p.scales[i].D && scales[i].Ns == p.scales[i].Ns);
		size_t slot = 0;
		for (size_t i = 0; i < nrows; i++) {
			if (ens[i] == NOSLOT) { REQUIRE(slot_of[i] == NOSLOT); continue; }
			REQUIRE(slot < nslots && slot_of[i] == slot && list[slot].row == i && list[slot].cls == p.cls_of[ens[i]]);
			// every partial entry a wave of this row writes lies inside the pass's partial block
			const FtClass &cl = p.classes[list[slot].cls];
			REQUIRE((slot * p.max_items + cl.nitems) * P * 16 <= ft_part_bytes(p, P, nslots));
			slot++;
		}
		REQUIRE(slot == nslots);
	}
	REQUIRE(next == B);
	// chunks of rows of the coefficient call
	const size_t nrow = B * M, chunk = ft_chunk_rows(nrow, p, P, budget);
	REQUIRE(chunk >= 1 && chunk <= nrow && (chunk == 1 || ft_pass_bytes(p, P, chunk) <= budget));
	if (chunk < nrow) REQUIRE(ft_pass_bytes(p, P, chunk + 1) > budget);
}

int main()
{
	std::mt19937_64 rng(20241020);
	unsigned long long nplans = 0, nrounds = 0;
	const size_t Ns[] = {1501, 2 * FT_SEG * 2 + 1, 64, 4096};
	for (size_t N : Ns)
		for (int odd = 0; odd < 2; odd++) {
			const Frame f = make_frame(N, 5, 3, odd != 0, rng);
			const unsigned S = (unsigned)f.sc.size();
			// edges that are no multiples of any D, at and around multiples of the decimations and of a segment of the finest scale, both trace ends
			const size_t e[] = {0, 1, 2, 3, 7, 8, 9, 37, 2 * FT_SEG - 1, 2 * FT_SEG, 2 * FT_SEG + 1, N / 2, N - 9, N - 1, N};
			const size_t ne = sizeof e / sizeof *e;
			std::vector<std::pair<size_t, size_t>> rg;
			for (size_t a = 0; a < ne; a++)
				for (size_t b = a + 1; b < ne; b++)
					if (e[a] < e[b] && e[b] <= N) rg.push_back({e[a], e[b]});
			const unsigned ranges[][2] = {{0, S}, {0, 1}, {3, 8}, {S - 1, S}};
			for (unsigned W = 1; W <= FT_WMAX; W++)
				for (size_t B : {(size_t)1, (size_t)2, (size_t)5})
					for (int rep = 0; rep < 12; rep++) {
						// B ensembles drawn from a few window sets, so that classes repeat; noise ranges that split or do not split a class
						std::vector<size_t> win(B * W * 2), noise;
						const size_t pool = 1 + rng() % 3, seed = rng();
						for (size_t b = 0; b < B; b++) {
							std::mt19937_64 g(seed + (rep % 2 ? b % pool : rng() % pool));
							for (unsigned w = 0; w < W; w++) { const auto &r = rg[g() % rg.size()]; win[(b * W + w) * 2] = r.first; win[(b * W + w) * 2 + 1] = r.second; }
						}
						if (rep % 3) {
							noise.resize(2 * B);
							for (size_t b = 0; b < B; b++) { const auto &r = rg[rep % 3 == 1 ? 5 : rng() % rg.size()]; noise[2 * b] = r.first; noise[2 * b + 1] = r.second; }
						}
						for (const auto &sr : ranges)
							for (int skip = 0; skip < 2; skip++) { check_plan(f, sr[0], sr[1], win, W, noise, B, skip); nplans++; }
					}
			// rounds and tables
			for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)40})
				for (size_t M : {(size_t)1, (size_t)9, (size_t)33}) {
					std::vector<size_t> win(B * 3 * 2), noise(B * 2);
					for (size_t b = 0; b < B; b++) {
						const size_t w3[6] = {3, N - 5, 0, N, N / 2 - (b % 2) * 7, N / 2 + 70};
						std::copy(w3, w3 + 6, &win[b * 6]);
						noise[2 * b] = b % 3; noise[2 * b + 1] = N / 4;
					}
					for (unsigned P : {1u, 3u, 4u}) {
						const FtPlan p = ft_plan(f.sc.data(), S, N, P == 3 ? 2 : 0, S, win.data(), 3, P == 1 ? nullptr : noise.data(), B, 1);
						const size_t one = ft_set_bytes(1, M, f.ncoef) + ft_pass_bytes(p, P, M), all = ft_set_bytes(B, M, f.ncoef) + ft_pass_bytes(p, P, B * M);
						for (int pattern = 0; pattern < 3; pattern++)
							for (size_t budget : {(size_t)1, one - 1, one, one + 1, 2 * one, 2 * one + one / 2, all - 1, all, (size_t)1 << 40}) {
								check_rounds(f, p, B, M, P, pattern, budget, rng);
								nrounds++;
							}
					}
				}
		}
	printf("%llu plans, %llu round plans, %llu checks: the classes, items, tasks, rounds and tables agree with the direct enumeration\n", nplans, nrounds, nchecks);
	return 0;
}
