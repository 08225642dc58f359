// mwcs_plan_check.cpp -- csrc/mwcs_plan.h against a direct enumeration, as a stand-alone program (built by `make -C ts-pws_amd
// mwcs_plan_check` with AddressSanitizer + UBSan; tests/test_mwcs_plan_cpu.py runs it).  It requires:
//   parameters  mw_par_error refuses exactly the sets outside the contract's ranges (each limit from both sides) and Qx > 64
//   bins        [qa, qb) = [max(0, q0 - h), min(P/2 + 1, q1 + h)); Qp the multiple of 16 at or above 2 Qx, Lp the multiple of 16 at or above L
//   windows     a start n belongs to range w iff n0 <= n, (n - n0) % hop == 0 and n + L <= n1, decided start by start; the list holds exactly
//               those, range after range in ascending n; j0 brackets them; mw_count_windows counts them; a range alone gives the same windows
//   basis       the layout's arrays tile the table (allocated at its exact size); Tc / Ts are the ascending-l sums of the entries; |C|, |S| <= g <= 1;
//               C^2 + S^2 = g^2 to rounding
//   rounds      the rounds tile the ensembles in order; spectra, window results and table stay within the budget unless the round is one
//               ensemble; a round that stops early could not have taken the next ensemble
//   table       every array of the block lies inside it, aligned, none overlapping (the block is allocated at its exact size: ASan sees any
//               write past it); Bt is the basis transposed with zero rows past L and zero columns past 2 Qx; the sources list each participating
//               row once, in order, with its ensemble, then the round's references; slot_of inverts it
#include "mwcs_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

static unsigned long long nchecks = 0;
#define REQUIRE(c)                                                                 \
	do {                                                                           \
		nchecks++;                                                                 \
		if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
	} while (0)

static MwPar good() { return {100, 37, 128, 3, 20, 2, 0.3, 0.5, 5.0, 20.0, 1e-3}; }

static void check_params()
{
	REQUIRE(!mw_par_error(good()));
	const double inf = INFINITY, nan = NAN;
	MwPar p;
#define BAD(stmt) do { p = good(); stmt; REQUIRE(mw_par_error(p) != nullptr); } while (0)
#define OK(stmt) do { p = good(); stmt; REQUIRE(mw_par_error(p) == nullptr); } while (0)
	BAD(p.L = 15); OK(p.L = 16; p.hop = 16); BAD(p.L = 1025; p.P = 2048); OK(p.L = 1024; p.P = 1024);
	BAD(p.hop = 0); OK(p.hop = 1); BAD(p.hop = 101); OK(p.hop = 100);
	BAD(p.P = 64); BAD(p.P = 96 * 2); BAD(p.P = 8192); OK(p.P = 4096); BAD(p.P = 0);
	BAD(p.q0 = 0); OK(p.q0 = 1); BAD(p.q0 = 19); OK(p.q0 = 18); BAD(p.q1 = 65); OK(p.q1 = 64; p.q0 = 40); BAD(p.q1 = 0); BAD(p.q1 = 1; p.q0 = 1);
	BAD(p.h = 9); OK(p.h = 8); OK(p.h = 0);
	BAD(p.taper = -0.1); BAD(p.taper = 1.5); BAD(p.taper = nan); OK(p.taper = 0.0); OK(p.taper = 1.0);
	BAD(p.min_coh = nan); BAD(p.max_err = nan); BAD(p.max_delta = nan); OK(p.max_err = inf; p.max_delta = inf);
	BAD(p.err_floor = 0.0); BAD(p.err_floor = -1.0); BAD(p.err_floor = nan); BAD(p.err_floor = inf);
	// Qx: 64 passes, 65 does not
	OK(p.L = 1024; p.hop = 1024; p.P = 1024; p.q0 = 20; p.q1 = 68; p.h = 8); BAD(p.L = 1024; p.hop = 1024; p.P = 1024; p.q0 = 20; p.q1 = 69; p.h = 8);
	OK(p.P = 128; p.q0 = 1; p.q1 = 64; p.h = 0); BAD(p.P = 128; p.q0 = 1; p.q1 = 64; p.h = 1); // (qa clips at 0, qb at P/2 + 1: 65 bins)
#undef BAD
#undef OK
}

static void check_bins_and_basis(const MwPar &p)
{
	const MwBins b = mw_bins(p);
	REQUIRE(b.qa == (p.q0 > p.h ? p.q0 - p.h : 0) && b.qb == std::min(p.P / 2 + 1, p.q1 + p.h) && b.Qx == b.qb - b.qa && b.Qx >= 2 && b.Qx <= MW_QMAX);
	REQUIRE(b.Qp % 16 == 0 && b.Qp >= 2 * b.Qx && b.Qp < 2 * b.Qx + 16 && b.Lp % 16 == 0 && b.Lp >= p.L && b.Lp < p.L + 16);
	const MwBasis o = mw_basis_layout(p);
	REQUIRE(o.g == 0 && o.C == p.L && o.S == o.C + (size_t)p.L * b.Qx && o.Tc == o.S + (size_t)p.L * b.Qx && o.Ts == o.Tc + b.Qx && o.k == o.Ts + b.Qx &&
	        o.v == o.k + 2 * p.h + 1 && o.doubles == o.v + b.Qx);
	std::vector<double> tab(o.doubles, -7.0);
	tab.shrink_to_fit();
	mw_basis(p, tab.data());
	for (unsigned q = 0; q < b.Qx; q++) {
		double tc = 0.0, ts = 0.0;
		for (unsigned l = 0; l < p.L; l++) {
			const double g = tab[o.g + l], c = tab[o.C + (size_t)l * b.Qx + q], s = tab[o.S + (size_t)l * b.Qx + q];
			REQUIRE(g > 0.0 && g <= 1.0 && fabs(c) <= g && fabs(s) <= g && fabs(c * c + s * s - g * g) <= 1e-15);
			REQUIRE(tab[o.g + l] == tab[o.g + p.L - 1 - l]);
			tc += c; ts += s;
		}
		REQUIRE(tc == tab[o.Tc + q] && ts == tab[o.Ts + q]);
		REQUIRE(tab[o.v + q] == (2.0 * M_PI) * (double)(b.qa + q) / (double)p.P);
	}
	for (unsigned d = 0; d <= 2 * p.h; d++) REQUIRE(tab[o.k + d] > 0.0 && tab[o.k + d] <= 1.0 && tab[o.k + d] == tab[o.k + 2 * p.h - d]);
	REQUIRE(tab[o.k + p.h] == 1.0);
}

static void check_windows(const std::vector<size_t> &win, size_t N, unsigned L, unsigned hop)
{
	const unsigned W = (unsigned)(win.size() / 2);
	const unsigned long long J = mw_count_windows(win.data(), W, L, hop);
	if (J > MW_JMAX) return;
	const MwWins wl = mw_windows(win.data(), W, L, hop);
	REQUIRE(wl.wins.size() == J && wl.j0[0] == 0);
	size_t at = 0;
	for (unsigned w = 0; w < W; w++) {
		REQUIRE(wl.j0[w] == at);
		for (size_t n = 0; n < N; n++) {
			const bool in = n >= win[2 * w] && (n - win[2 * w]) % hop == 0 && n + L <= win[2 * w + 1];
			if (in) { REQUIRE(at < wl.wins.size() && wl.wins[at].n0 == n && wl.wins[at].w == w); at++; }
		}
		const MwWins one = mw_windows(&win[2 * w], 1, L, hop);
		REQUIRE(one.wins.size() == at - wl.j0[w]);
		for (size_t j = 0; j < one.wins.size(); j++) REQUIRE(one.wins[j].n0 == wl.wins[wl.j0[w] + j].n0);
	}
	for (unsigned w = W; w <= MW_WMAX; w++) REQUIRE(wl.j0[w] == at);
	REQUIRE(at == wl.wins.size());
}

static void check_rounds(const MwPar &p, const std::vector<size_t> &win, size_t B, size_t M, int pattern, size_t budget, std::mt19937_64 &rng)
{
	const unsigned W = (unsigned)(win.size() / 2);
	const MwWins wl = mw_windows(win.data(), W, p.L, p.hop);
	const size_t J = wl.wins.size();
	const MwBins b = mw_bins(p);
	const MwBasis bo = mw_basis_layout(p);
	std::vector<double> basis(bo.doubles);
	mw_basis(p, basis.data());
	std::vector<unsigned> mtr(B * M);
	for (auto &c : mtr) c = pattern == 2 ? 0 : pattern == 1 ? (unsigned)(rng() % 3) : 5;
	std::vector<size_t> nrows0(B + 1, 0);
	for (size_t e = 0; e < B; e++) {
		size_t n = 0;
		for (size_t m = 0; m < M; m++) n += mtr[e * M + m] > 0;
		nrows0[e + 1] = nrows0[e] + n;
	}
	const std::vector<Round> rounds = mw_rounds(B, nrows0.data(), M, J, p, budget);
	size_t next = 0;
	for (const Round &r : rounds) {
		REQUIRE(r.j0 == next && r.j1 > r.j0 && r.j1 <= B);
		next = r.j1;
		REQUIRE(mw_round_bytes(nrows0.data(), r.j0, r.j1, M, J, p) <= budget || r.j1 - r.j0 == 1);
		if (r.j1 < B) REQUIRE(mw_round_bytes(nrows0.data(), r.j0, r.j1 + 1, M, J, p) > budget);
		const size_t nb = r.j1 - r.j0, nrows = nrows0[r.j1] - nrows0[r.j0];
		REQUIRE(mw_round_bytes(nrows0.data(), r.j0, r.j1, M, J, p) == (nrows + nb) * J * b.Qp * 8 + nrows * J * 24 + mw_tab(p, J, nrows + nb, nb * M).bytes);
		const MwTab t = mw_tab(p, J, nrows + nb, nb * M);
		const size_t off[8] = {t.bt, t.T, t.k, t.v, t.wins, t.srcs, t.slot_of, t.bytes};
		const size_t size[7] = {(size_t)b.Qp * b.Lp * 8, (size_t)b.Qp * 8, (size_t)(2 * p.h + 1) * 8, (size_t)b.Qx * 8, J * sizeof(MwWin), (nrows + nb) * sizeof(MwSrc), nb * M * 4};
		const size_t align[7] = {8, 8, 8, 8, alignof(MwWin), alignof(MwSrc), 4};
		for (int i = 0; i < 7; i++) REQUIRE(off[i] % align[i] == 0 && off[i] + size[i] <= off[i + 1] && off[i + 1] <= t.bytes);
		REQUIRE(t.bt % 32 == 0 && ((size_t)b.Lp * 8) % 32 == 0); // (the kernel loads 32-byte vectors of a column at multiples of 4 rows)
		std::vector<char> blob(std::max<size_t>(t.bytes, 1), 0);
		blob.shrink_to_fit();
		REQUIRE(mw_fill_round(blob.data(), t, r, M, pattern == 0 ? nullptr : mtr.data(), p, basis.data(), wl) == nrows);
		const double *bt = (const double *)(blob.data() + t.bt), *T = (const double *)(blob.data() + t.T);
		for (unsigned c = 0; c < b.Qp; c++) {
			for (unsigned l = 0; l < b.Lp; l++) {
				const double want = l >= p.L || c >= 2 * b.Qx ? 0.0 : c < b.Qx ? basis[bo.C + (size_t)l * b.Qx + c] : basis[bo.S + (size_t)l * b.Qx + c - b.Qx];
				REQUIRE(bt[(size_t)c * b.Lp + l] == want);
			}
			REQUIRE(T[c] == (c >= 2 * b.Qx ? 0.0 : c < b.Qx ? basis[bo.Tc + c] : basis[bo.Ts + c - b.Qx]));
		}
		const double *k = (const double *)(blob.data() + t.k), *v = (const double *)(blob.data() + t.v);
		for (unsigned d = 0; d <= 2 * p.h; d++) REQUIRE(k[d] == basis[bo.k + d]);
		for (unsigned q = 0; q < b.Qx; q++) REQUIRE(v[q] == basis[bo.v + q]);
		const MwWin *dw = (const MwWin *)(blob.data() + t.wins);
		for (size_t j = 0; j < J; j++) REQUIRE(dw[j].n0 == wl.wins[j].n0 && dw[j].w == wl.wins[j].w);
		const MwSrc *srcs = (const MwSrc *)(blob.data() + t.srcs);
		const unsigned *slot_of = (const unsigned *)(blob.data() + t.slot_of);
		size_t slot = 0;
		for (size_t e = r.j0; e < r.j1; e++)
			for (size_t m = 0; m < M; m++) {
				const size_t i = (e - r.j0) * M + m;
				if (mtr[e * M + m] == 0) { REQUIRE(slot_of[i] == NOSLOT); continue; }
				REQUIRE(slot < nrows && slot_of[i] == slot && srcs[slot].row == e * M + m && srcs[slot].bl == e - r.j0);
				slot++;
			}
		REQUIRE(slot == nrows);
		for (size_t e = r.j0; e < r.j1; e++) REQUIRE(srcs[nrows + e - r.j0].row == e && srcs[nrows + e - r.j0].bl == MW_REF);
	}
	REQUIRE(next == B);
}

int main()
{
	std::mt19937_64 rng(20241101);
	unsigned long long nwin = 0, nrounds = 0;
	check_params();
	const MwPar sets[] = {good(), {1024, 1024, 1024, 20, 68, 8, 0.1, 0.2, INFINITY, INFINITY, 1e-4}, {16, 1, 16, 1, 3, 2, 1.0, 0.3, 50.0, INFINITY, 1e-2},
	                      {512, 128, 512, 40, 72, 4, 0.15, 0.5, INFINITY, INFINITY, 1e-3}, {17, 5, 4096, 2000, 2048, 8, 0.0, 0.0, 1.0, 1.0, 1.0}};
	for (const MwPar &p : sets) { REQUIRE(!mw_par_error(p)); check_bins_and_basis(p); }
	const size_t N = 1501;
	const size_t e[] = {0, 1, 3, 15, 16, 17, 99, 100, 101, 137, 611, 661, 700, 712, N - 100, N - 16, N - 1, N};
	const size_t ne = sizeof e / sizeof *e;
	const unsigned LH[][2] = {{100, 37}, {16, 1}, {16, 16}, {1024, 1024}, {17, 5}, {100, 100}, {512, 128}};
	for (const auto &lh : LH) {
		for (size_t a = 0; a < ne; a++)
			for (size_t c = a + 1; c < ne; c++) { check_windows({e[a], e[c]}, N, lh[0], lh[1]); nwin++; }
		check_windows({0, N, 700, 712, 661, N, 3, 611}, N, lh[0], lh[1]);
		check_windows({3, 611, 3, 611, 0, 16}, N, lh[0], lh[1]);
		nwin += 2;
	}
	const std::vector<size_t> win = {0, N, 700, 712, 661, N, 3, 611};
	for (const MwPar &p : {sets[0], sets[1], sets[4]})
		for (size_t B : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)40})
			for (size_t M : {(size_t)1, (size_t)9, (size_t)33}) {
				std::vector<size_t> full(B + 1);
				for (size_t i = 0; i <= B; i++) full[i] = i * M;
				const size_t J = mw_windows(win.data(), 4, p.L, p.hop).wins.size();
				const size_t one = mw_round_bytes(full.data(), 0, 1, M, J, p), all = mw_round_bytes(full.data(), 0, B, M, J, p);
				for (int pattern = 0; pattern < 3; pattern++)
					for (size_t budget : {(size_t)1, one - 1, one, one + 1, 2 * one, 2 * one + one / 2, all - 1, all, (size_t)1 << 40}) {
						check_rounds(p, win, B, M, pattern, budget, rng);
						nrounds++;
					}
			}
	printf("%llu window lists, %llu round plans, %llu checks: the parameters, bins, windows, basis, rounds and tables agree with the direct enumeration\n", nwin,
	       nrounds, nchecks);
	return 0;
}
