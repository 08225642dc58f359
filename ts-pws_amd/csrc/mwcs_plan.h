// mwcs_plan.h -- how tspws_hip_mwcs_rows (mwcs_rows.hip) cuts its work: the parameter check, the extended bin range, the window list, the
// basis table (tspws_mwcs_basis), the rounds of whole ensembles that keep the spectra and the per-window results inside the parts budget, and
// the ONE table block a round uploads.  Host code only, no HIP runtime: tests/mwcs_plan_check.cpp compiles it with a plain C++17 compiler.
//
// BINS.  The band [q0, q1) extended by the smoothing half-width: [qa, qb) = [max(0, q0 - h), min(P/2 + 1, q1 + h)), Qx = qb - qa <= 64.  The
// contraction has 2 Qx columns (Qx cosine columns, then Qx sine columns) padded with zero columns to Qp, a multiple of 16.
// WINDOWS.  Range w = [n0, n1) holds J_w = (n1 - n0 >= L) ? (n1 - n0 - L) / hop + 1 : 0 windows at n0 + j hop, numbered range after range:
// the windows of range w are [j0[w], j0[w + 1]).  A window depends on its range, L and hop alone.
// ITEMS.  A source is a participating row of the round (slots [0, nrows), in row order) or the reference of one of its ensembles (slots
// [nrows, nrows + nb)); an item is (source, window), numbered slot J + j.  A wave of the contraction takes MW_ROWS consecutive items: an item's
// spectrum depends on its own samples alone, so a tile may straddle rows, ensembles and ranges.
// ROUNDS.  Whole ensembles whose spectra ((rows + 1) J Qp doubles each), per-window results (rows J 3 doubles) and table stay inside the parts
// budget; the first ensemble of a round is always taken (one alone may exceed the budget).  The round rule, participation, the slots and the
// range words are host_plan.h's.
#pragma once

#include "host_plan.h"

#include <cmath>
#include <cstdint>

enum { MW_WMAX = 4, MW_JMAX = 4096, MW_QMAX = 64, MW_LMIN = 16, MW_LMAX = 1024, MW_PMAX = 4096, MW_HMAX = 8, MW_ROWS = 32, MW_CT = 16, MW_NT = 4 };
constexpr unsigned MW_REF = ~0u;

struct MwPar { unsigned L, hop, P, q0, q1, h; double taper, min_coh, max_err, max_delta, err_floor; }; // (tspws_mwcs_par)
struct MwBins { unsigned qa, qb, Qx, Qp, Lp; }; // Qp: padded columns, Lp: L rounded up to 16 (the table's rows past L are zero)
struct MwWin { unsigned n0, w; };               // window: first sample, range
struct MwSrc { unsigned row, bl; };             // a row: its index b M + m in d_rows and its ensemble's index in the round; a reference: (b, MW_REF)

// what is wrong with the parameters (NULL: nothing); needs no plan
inline const char *mw_par_error(const MwPar &p)
{
	if (p.L < MW_LMIN || p.L > MW_LMAX) return "a window length outside [16, 1024]";
	if (p.hop < 1 || p.hop > p.L) return "a hop outside [1, L]";
	if (p.P < p.L || p.P > MW_PMAX || (p.P & (p.P - 1))) return "a DFT length that is no power of two in [L, 4096]";
	if (p.q0 < 1 || p.q1 > p.P / 2 || p.q1 < 2 || p.q0 > p.q1 - 2) return "a band outside 1 <= q0, q0 + 2 <= q1 <= P / 2";
	if (p.h > MW_HMAX) return "a smoothing half-width above 8";
	if (!(p.taper >= 0.0 && p.taper <= 1.0)) return "a taper fraction outside [0, 1]";
	if (std::isnan(p.min_coh) || std::isnan(p.max_err) || std::isnan(p.max_delta)) return "a NaN filter";
	if (!(p.err_floor > 0.0) || !std::isfinite(p.err_floor)) return "an error floor that is not positive and finite";
	const unsigned qa = p.q0 > p.h ? p.q0 - p.h : 0, qb = std::min(p.P / 2 + 1, p.q1 + p.h);
	if (qb - qa > MW_QMAX) return "more than 64 bins with the smoothing margins";
	return nullptr;
}

inline MwBins mw_bins(const MwPar &p)
{
	MwBins b;
	b.qa = p.q0 > p.h ? p.q0 - p.h : 0;
	b.qb = std::min(p.P / 2 + 1, p.q1 + p.h);
	b.Qx = b.qb - b.qa;
	b.Qp = (2 * b.Qx + MW_CT - 1) / MW_CT * MW_CT;
	b.Lp = (p.L + 15u) & ~15u;
	return b;
}

// windows of the ranges win[2 w], win[2 w + 1] (n0 < n1, checked by the caller), without building them: sum of J_w
inline unsigned long long mw_count_windows(const size_t *win, unsigned W, unsigned L, unsigned hop)
{
	unsigned long long J = 0;
	for (unsigned w = 0; w < W; w++) {
		const size_t len = win[2 * w + 1] - win[2 * w];
		if (len >= L) J += (len - L) / hop + 1;
	}
	return J;
}

struct MwWins {
	std::vector<MwWin> wins;
	unsigned j0[MW_WMAX + 1] = {0, 0, 0, 0, 0}; // the windows of range w: [j0[w], j0[w + 1])
};
// (n1 <= N < 2^32 and J <= MW_JMAX checked by the caller)
inline MwWins mw_windows(const size_t *win, unsigned W, unsigned L, unsigned hop)
{
	MwWins o;
	for (unsigned w = 0; w < W; w++) {
		o.j0[w] = (unsigned)o.wins.size();
		for (size_t n = win[2 * w]; n + L <= win[2 * w + 1]; n += hop) o.wins.push_back({(unsigned)n, w});
	}
	for (unsigned w = W; w <= MW_WMAX; w++) o.j0[w] = (unsigned)o.wins.size();
	return o;
}

// ---- the basis (tspws_mwcs_basis) -----------------------------------------------------------------------------------------------------
// tab = g[L] | C[L][Qx] | S[L][Qx] | Tc[Qx] | Ts[Qx] | k[2 h + 1] | v[Qx] doubles
struct MwBasis { size_t g, C, S, Tc, Ts, k, v, doubles; };
inline MwBasis mw_basis_layout(const MwPar &p)
{
	const MwBins b = mw_bins(p);
	MwBasis o;
	o.g = 0; o.C = o.g + p.L; o.S = o.C + (size_t)p.L * b.Qx; o.Tc = o.S + (size_t)p.L * b.Qx; o.Ts = o.Tc + b.Qx; o.k = o.Ts + b.Qx; o.v = o.k + 2 * p.h + 1;
	o.doubles = o.v + b.Qx;
	return o;
}

// g[l]: with a = taper L / 2 samples under each flank and x = min(l + 1/2, L - 1/2 - l): 0.5 (1 - cos(PI x / a)) for x < a, else 1.
// Every entry of g, C and S is evaluated in long double and rounded to double ONCE (C and S: the product of the rounded g[l] and the
// long double cosine / sine of the exact angle 2 PI m / P, m = (q l) mod P); Tc and Ts add the rounded entries in ascending l in double.
inline void mw_basis(const MwPar &p, double *tab)
{
	const MwBins b = mw_bins(p);
	const MwBasis o = mw_basis_layout(p);
	const long double pi = 3.14159265358979323846264338327950288L;
	const double a = p.taper * (double)p.L * 0.5;
	for (unsigned l = 0; l < p.L; l++) {
		const double x = std::min((double)l + 0.5, ((double)p.L - 0.5) - (double)l);
		tab[o.g + l] = x < a ? (double)(0.5L * (1.0L - cosl(pi * (long double)x / (long double)a))) : 1.0;
	}
	// the P distinct angles once (q l runs through them L Qx times)
	std::vector<long double> cs(p.P), sn(p.P);
	for (unsigned m = 0; m < p.P; m++) {
		const long double ang = 2.0L * pi * (long double)m / (long double)p.P;
		cs[m] = cosl(ang); sn[m] = sinl(ang);
	}
	for (unsigned q = 0; q < b.Qx; q++) { tab[o.Tc + q] = 0.0; tab[o.Ts + q] = 0.0; }
	for (unsigned l = 0; l < p.L; l++)
		for (unsigned q = 0; q < b.Qx; q++) {
			const unsigned m = (unsigned)(((unsigned long long)(b.qa + q) * l) % p.P);
			const long double g = (long double)tab[o.g + l];
			const double c = (double)(g * cs[m]), s = (double)(-(g * sn[m]));
			tab[o.C + (size_t)l * b.Qx + q] = c;
			tab[o.S + (size_t)l * b.Qx + q] = s;
			tab[o.Tc + q] += c;
			tab[o.Ts + q] += s;
		}
	for (unsigned d = 0; d <= 2 * p.h; d++) tab[o.k + d] = 0.5 * (1.0 + cos(M_PI * ((double)d - (double)p.h) / (double)(p.h + 1)));
	for (unsigned q = 0; q < b.Qx; q++) tab[o.v + q] = (2.0 * M_PI) * (double)(b.qa + q) / (double)p.P;
}

// ---- the table block of a round ------------------------------------------------------------------------------------------------------
// Bt[Qp][Lp] (column c < Qx: C[.][c]; Qx <= c < 2 Qx: S[.][c - Qx]; the rest and the rows past L zero) | T[Qp] (Tc | Ts | zero) | k[2 h + 1] | v[Qx] |
// windows | sources | slot of every (ensemble of the round, m) or NOSLOT
struct MwTab { size_t bt, T, k, v, wins, srcs, slot_of, bytes; };
inline MwTab mw_tab(const MwPar &p, size_t J, size_t nsrc, size_t nall)
{
	const MwBins b = mw_bins(p);
	TableLayout lay;
	MwTab t;
	t.bt = lay.add<double>((size_t)b.Qp * b.Lp); t.T = lay.add<double>(b.Qp); t.k = lay.add<double>(2 * p.h + 1); t.v = lay.add<double>(b.Qx);
	t.wins = lay.add<MwWin>(J); t.srcs = lay.add<MwSrc>(nsrc); t.slot_of = lay.add<unsigned>(nall);
	t.bytes = lay.bytes;
	return t;
}

// the device blocks of a round, in bytes: the spectra F[slot J + j][Qp] of rows and references, the results win[slot J + j][3] of the rows
inline size_t mw_spec_bytes(size_t nb, size_t nrows, size_t J, const MwBins &b) { return (nrows + nb) * J * b.Qp * sizeof(double); }
inline size_t mw_win_bytes(size_t nrows, size_t J) { return nrows * J * 3 * sizeof(double); }
// nrows0: participating_rows0
inline size_t mw_round_bytes(const size_t *nrows0, size_t j0, size_t j1, size_t M, size_t J, const MwPar &p)
{
	const size_t nb = j1 - j0, nrows = nrows0[j1] - nrows0[j0];
	return mw_spec_bytes(nb, nrows, J, mw_bins(p)) + mw_win_bytes(nrows, J) + mw_tab(p, J, nrows + nb, nb * M).bytes;
}

inline std::vector<Round> mw_rounds(size_t B, const size_t *nrows0, size_t M, size_t J, const MwPar &p, size_t budget)
{
	return whole_ensemble_rounds(B, [&](size_t j0, size_t j1) { return mw_round_bytes(nrows0, j0, j1, M, J, p) <= budget; });
}

// the table of round r into blob (mw_tab's layout with the round's own counts; zeroed by the caller); basis: mw_basis's table.  Returns the
// participating rows.
inline size_t mw_fill_round(char *blob, const MwTab &t, const Round &r, size_t M, const unsigned *h_mtr, const MwPar &p, const double *basis, const MwWins &wl)
{
	const MwBins b = mw_bins(p);
	const MwBasis o = mw_basis_layout(p);
	double *bt = (double *)(blob + t.bt), *T = (double *)(blob + t.T);
	for (unsigned q = 0; q < b.Qx; q++) {
		for (unsigned l = 0; l < p.L; l++) {
			bt[(size_t)q * b.Lp + l] = basis[o.C + (size_t)l * b.Qx + q];
			bt[(size_t)(b.Qx + q) * b.Lp + l] = basis[o.S + (size_t)l * b.Qx + q];
		}
		T[q] = basis[o.Tc + q];
		T[b.Qx + q] = basis[o.Ts + q];
	}
	std::copy(basis + o.k, basis + o.k + 2 * p.h + 1, (double *)(blob + t.k));
	std::copy(basis + o.v, basis + o.v + b.Qx, (double *)(blob + t.v));
	std::copy(wl.wins.begin(), wl.wins.end(), (MwWin *)(blob + t.wins));
	MwSrc *srcs = (MwSrc *)(blob + t.srcs);
	const size_t slot = fill_round_slots((unsigned *)(blob + t.slot_of), r, M, h_mtr,
	                                     [&](size_t s, size_t e, size_t m) { srcs[s] = {(unsigned)(e * M + m), (unsigned)(e - r.j0)}; });
	for (size_t e = r.j0; e < r.j1; e++) srcs[slot + (e - r.j0)] = {(unsigned)e, MW_REF};
	return slot;
}
