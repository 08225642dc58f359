// wxs_plan_check.cpp -- csrc/wxs_plan.h against a direct per-coefficient enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// wxs_plan_check` with AddressSanitizer + UBSan; tests/test_wxs_plan_cpu.py runs it).  It requires:
//   scales   `used` holds exactly the scales inside at least one band, increasing, and uidx inverts it
//   items    for every (scale in use, window) the coefficients k with n0 <= k D < n1 -- and, under the wrap rule, with their filter support
//            [k D - c, k D - c + L) inside [0, N), decided per coefficient -- are exactly the ones the span's items hold, each once, at
//            coef_off + k; the items of a span start at the range's first index plus multiples of WX_SEG (they depend on that scale and window
//            alone: the plan of one band or one window alone gives the same items), hold 1 .. WX_SEG coefficients, and carry D and omega;
//            no item belongs to a scale out of use
//   tasks    the tasks tile the items in order, each of at most WX_TASK passes, and no task could have taken the next item
//   rounds   the rounds tile the ensembles in order; sets, partial sums and table stay within the budget unless the round is one ensemble;
//            a round that stops early could not have taken the next ensemble; a chunk of rows fits or is one row, and one more would not fit
//   table    every array of the block lies inside it, aligned, none overlapping (the block is allocated at its exact size: ASan sees any
//            write past it); the list holds each participating row once, in order, with its reference; slot_of inverts it
#include "wxs_plan.h"

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
			s.omega = 6.0 / (2.0 * (1u << j) * (1.0 + 0.25 * v));
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

static bool same_item(const WxItem &a, const WxItem &b) { return a.coef == b.coef && a.k0 == b.k0 && a.count == b.count && a.D == b.D && a.omega == b.omega; }

static void check_plan(const Frame &f, const std::vector<WxBand> &bands, const std::vector<size_t> &win, int skip)
{
	const unsigned S = (unsigned)f.sc.size(), R = (unsigned)bands.size(), W = (unsigned)(win.size() / 2);
	const WxPlan p = wx_plan(f.sc.data(), S, f.N, bands.data(), R, win.data(), W, skip);
	REQUIRE(p.W == W && p.uidx.size() == S && p.spans.size() == p.used.size() * W);
	unsigned u = 0;
	for (unsigned s = 0; s < S; s++) {
		bool in = false;
		for (const WxBand &b : bands) in = in || (s >= b.s_begin && s < b.s_end);
		if (in) { REQUIRE(u < p.used.size() && p.used[u] == s && p.uidx[s] == u); u++; }
		else REQUIRE(p.uidx[s] == NOSLOT);
	}
	REQUIRE(u == p.used.size());
	unsigned next = 0;
	for (u = 0; u < p.used.size(); u++) {
		const WxScale &s = f.sc[p.used[u]];
		for (unsigned w = 0; w < W; w++) {
			const WxSpan sp = p.spans[(size_t)u * W + w];
			REQUIRE(sp.first == next);
			next += sp.n;
			std::vector<unsigned char> seen(s.Ns, 0);
			size_t first = s.Ns;
			for (size_t k = 0; k < s.Ns; k++)
				if (takes_part(s, f.N, k, win[2 * w], win[2 * w + 1], skip)) { first = k; break; }
			for (unsigned i = 0; i < sp.n; i++) {
				REQUIRE(sp.first + i < p.items.size());
				const WxItem &it = p.items[sp.first + i];
				REQUIRE(it.count >= 1 && it.count <= WX_SEG && it.k0 == first + (size_t)i * WX_SEG && it.coef == s.coef_off + it.k0);
				REQUIRE(it.D == s.D && it.omega == s.omega && (size_t)it.k0 + it.count <= s.Ns && it.coef + it.count <= f.ncoef);
				REQUIRE(i + 1 == sp.n || it.count == WX_SEG);
				for (unsigned j = 0; j < it.count; j++) { REQUIRE(!seen[it.k0 + j]); seen[it.k0 + j] = 1; }
			}
			for (size_t k = 0; k < s.Ns; k++) REQUIRE(seen[k] == takes_part(s, f.N, k, win[2 * w], win[2 * w + 1], skip));
			// the same items from this window alone and this scale alone
			const WxBand one = {p.used[u], p.used[u] + 1};
			const WxPlan q = wx_plan(f.sc.data(), S, f.N, &one, 1, &win[2 * w], 1, skip);
			REQUIRE(q.used.size() == 1 && q.spans.size() == 1 && q.spans[0].n == sp.n && q.items.size() == sp.n);
			for (unsigned i = 0; i < sp.n; i++) REQUIRE(same_item(q.items[i], p.items[sp.first + i]));
		}
	}
	REQUIRE(next == p.items.size());
	next = 0;
	for (size_t t = 0; t < p.tasks.size(); t++) {
		const WxTask &tk = p.tasks[t];
		REQUIRE(tk.first == next && tk.n >= 1 && tk.first + tk.n <= p.items.size());
		unsigned passes = 0;
		for (unsigned i = 0; i < tk.n; i++) passes += (p.items[tk.first + i].count + 63) / 64;
		REQUIRE(passes <= WX_TASK);
		next += tk.n;
		if (next < p.items.size()) REQUIRE(passes + (p.items[next].count + 63) / 64 > WX_TASK);
	}
	REQUIRE(next == p.items.size());
}

static void check_rounds(const Frame &f, const WxPlan &p, const std::vector<WxBand> &bands, size_t B, size_t M, int pattern, size_t budget, std::mt19937_64 &rng)
{
	const unsigned R = (unsigned)bands.size();
	auto total = [&](size_t nb) { return wx_set_bytes(nb, M, f.ncoef) + wx_pass_bytes(p, R, nb * M); };
	const std::vector<Round> rounds = wx_rounds(B, M, f.ncoef, p, R, budget);
	size_t next = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= B);
		next = r.j1;
		REQUIRE(total(r.j1 - r.j0) <= budget || r.j1 - r.j0 == 1);
		if (r.j1 < B) REQUIRE(total(r.j1 + 1 - r.j0) > budget);
		// the table of the round, in a block of its exact size
		const size_t nrows = (r.j1 - r.j0) * M;
		std::vector<unsigned> ens(nrows);
		for (size_t i = 0; i < nrows; i++) ens[i] = pattern == 2 || (pattern == 1 && rng() % 3 == 0) ? NOSLOT : (unsigned)(i / M);
		const size_t nslots = count_slots(ens.data(), nrows);
		const WxTab t = wx_tab(p, R, nslots, nrows);
		const size_t off[8] = {t.items, t.tasks, t.spans, t.uidx, t.bands, t.list, t.slot_of, t.bytes};
		const size_t size[7] = {p.items.size() * sizeof(WxItem), p.tasks.size() * sizeof(WxTask), p.spans.size() * sizeof(WxSpan), p.uidx.size() * sizeof(unsigned),
		                        R * sizeof(WxBand), nslots * sizeof(WxRow), nrows * sizeof(unsigned)};
		const size_t align[7] = {alignof(WxItem), alignof(WxTask), alignof(WxSpan), alignof(unsigned), alignof(WxBand), alignof(WxRow), alignof(unsigned)};
		for (int i = 0; i < 7; i++) REQUIRE(off[i] % align[i] == 0 && off[i] + size[i] <= off[i + 1] && off[i + 1] <= t.bytes);
		REQUIRE(t.bytes <= wx_tab(p, R, nrows, nrows).bytes && wx_part_bytes(p, nslots) + t.bytes <= wx_pass_bytes(p, R, nrows));
		std::vector<char> blob(std::max<size_t>(t.bytes, 1), 0);
		blob.shrink_to_fit();
		REQUIRE(wx_fill(blob.data(), t, p, bands.data(), R, ens.data(), nrows) == nslots);
		const WxItem *items = (const WxItem *)(blob.data() + t.items);
		const WxTask *tasks = (const WxTask *)(blob.data() + t.tasks);
		const WxSpan *spans = (const WxSpan *)(blob.data() + t.spans);
		const unsigned *uidx = (const unsigned *)(blob.data() + t.uidx), *slot_of = (const unsigned *)(blob.data() + t.slot_of);
		const WxBand *bd = (const WxBand *)(blob.data() + t.bands);
		const WxRow *list = (const WxRow *)(blob.data() + t.list);
		for (size_t i = 0; i < p.items.size(); i++) REQUIRE(same_item(items[i], p.items[i]));
		for (size_t i = 0; i < p.tasks.size(); i++) REQUIRE(tasks[i].first == p.tasks[i].first && tasks[i].n == p.tasks[i].n);
		for (size_t i = 0; i < p.spans.size(); i++) REQUIRE(spans[i].first == p.spans[i].first && spans[i].n == p.spans[i].n);
		for (size_t i = 0; i < p.uidx.size(); i++) REQUIRE(uidx[i] == p.uidx[i]);
		for (unsigned i = 0; i < R; i++) REQUIRE(bd[i].s_begin == bands[i].s_begin && bd[i].s_end == bands[i].s_end);
		size_t slot = 0;
		for (size_t i = 0; i < nrows; i++) {
			if (ens[i] == NOSLOT) { REQUIRE(slot_of[i] == NOSLOT); continue; }
			REQUIRE(slot < nslots && slot_of[i] == slot && list[slot].row == i && list[slot].ens == ens[i]);
			slot++;
		}
		REQUIRE(slot == nslots);
	}
	REQUIRE(next == B);
	// chunks of rows of the coefficient call
	const size_t nrow = B * M, chunk = wx_chunk_rows(nrow, p, R, budget);
	REQUIRE(chunk >= 1 && chunk <= nrow && (chunk == 1 || wx_pass_bytes(p, R, chunk) <= budget));
	if (chunk < nrow) REQUIRE(wx_pass_bytes(p, R, chunk + 1) > budget);
}

int main()
{
	std::mt19937_64 rng(20240913);
	unsigned long long nplans = 0, nrounds = 0;
	const size_t Ns[] = {1501, 2 * WX_SEG * 2 + 1, 64, 4096};
	for (size_t N : Ns)
		for (int odd = 0; odd < 2; odd++) {
			const Frame f = make_frame(N, 5, 3, odd != 0, rng);
			const unsigned S = (unsigned)f.sc.size();
			// bands: one octave, one cut between voices, two overlapping, one empty; all scales; one scale; the last scales
			const std::vector<std::vector<WxBand>> tables = {{{3, 6}, {4, 8}, {0, 5}, {2, 9}, {7, 7}}, {{0, S}}, {{1, 2}}, {{S - 2, S}, {0, 0}}, {{S, S}}};
			// windows: edges that are no multiples of any D, at and around multiples of the decimations and of a segment of the finest scale, both trace ends
			const size_t e[] = {0, 1, 2, 3, 7, 8, 9, 37, 2 * WX_SEG - 1, 2 * WX_SEG, 2 * WX_SEG + 1, N / 2, N - 9, N - 1, N};
			const size_t ne = sizeof e / sizeof *e;
			std::vector<std::vector<size_t>> wins;
			for (size_t a = 0; a < ne; a++)
				for (size_t b = a + 1; b < ne; b++)
					if (e[a] < e[b] && e[b] <= N) wins.push_back({e[a], e[b]});
			wins.push_back({3, N - 5, 0, N, 5, 6});
			wins.push_back({N / 3, 2 * N / 3 + 1, N / 2, N, 0, N / 2 + 3, 1, 2});
			for (const auto &bands : tables)
				for (const auto &win : wins)
					for (int skip = 0; skip < 2; skip++) { check_plan(f, bands, win, skip); nplans++; }
			// rounds and tables
			const std::vector<size_t> win = {3, N - 5, 0, N, N / 2, N / 2 + 70};
			for (const auto &bands : tables) {
				const unsigned R = (unsigned)bands.size();
				const WxPlan p = wx_plan(f.sc.data(), S, N, bands.data(), R, win.data(), 3, 1);
				for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)40})
					for (size_t M : {(size_t)1, (size_t)9, (size_t)33}) {
						const size_t one = wx_set_bytes(1, M, f.ncoef) + wx_pass_bytes(p, R, M), all = wx_set_bytes(B, M, f.ncoef) + wx_pass_bytes(p, R, B * M);
						for (int pattern = 0; pattern < 3; pattern++)
							for (size_t budget : {(size_t)1, one - 1, one, one + 1, 2 * one, 2 * one + one / 2, all - 1, all, (size_t)1 << 40}) {
								check_rounds(f, p, bands, B, M, pattern, budget, rng);
								nrounds++;
							}
					}
			}
		}
	printf("%llu plans, %llu round plans, %llu checks: the scales, items, tasks, rounds and tables agree with the direct enumeration\n", nplans, nrounds, nchecks);
	return 0;
}
