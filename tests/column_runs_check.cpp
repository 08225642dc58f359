// column_runs_check.cpp -- the run tables of the two-stage replicas (csrc/column_runs.h, csrc/masked_tables.h) against the per-trace definition,
// on the CPU.  Built with AddressSanitizer + UBSan and run by tests/test_column_runs_cpu.py; prints one summary line, exit status 1 at the
// first failed check.
//
// The definition, computed here trace by trace and independently of pieces: the group of trace i in replica c is floor(k KM / max(K_c, 1)),
// k = its rank among the bytes == 1 of the column (any other byte: deleted); the plain stack's is min(floor(i KM / m), KM - 1).
// Every trace carries a random 64-bit integer, and each table form is simulated in wrap-around integer arithmetic by the contract that its
// kernel's comment states (stream.hip: k_rows_walk + k_seg_fix, k_prefix_walk + k_combine_terms; jk_batch_two_stage.hip: k_jb2_rows_walk):
// every row must equal the sum of the traces of its (column, group), and the rows never stored must be exactly those without a trace.
#include "masked_tables.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

typedef uint64_t u64;

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { u64 z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static char case_text[256];
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n  case: %s\n", __FILE__, __LINE__, #cond, case_text); exit(1); } } while (0)

static const unsigned NONE = ~0u;

struct Case {
	size_t m = 0;
	unsigned KM = 0, C = 0, W = 0;
	bool with_main = false;
	std::vector<char> sel;               // [C][m]
	std::vector<std::vector<unsigned>> grp; // [W][m]: the definition
	std::vector<size_t> Kc;
	std::vector<u64> x;                  // a number per trace
};

// column patterns (the module docstring of test_column_runs_cpu.py lists them)
static void fill_column(char *row, size_t m, unsigned KM, unsigned pattern, unsigned variant)
{
	for (size_t i = 0; i < m; i++) row[i] = 0;
	switch (pattern % 7) {
	case 0: for (size_t i = 0; i < m; i++) row[i] = 1; break;                      // all kept
	case 1: break;                                                                  // all deleted
	case 2: for (unsigned k = 0; k + 1 < KM && k < m; k++) row[rnd() % m] = 1; break; // fewer kept traces than groups
	case 3: for (size_t i = variant & 1; i < m; i += 2) row[i] = 1; break;          // alternating
	case 4: {                                                                       // one kept stretch of 8, 9 or 17 bytes at offset 0..7
		const size_t len = variant % 3 == 0 ? 8 : variant % 3 == 1 ? 9 : 17, off = (variant / 3) % 8;
		for (size_t i = off; i < off + len && i < m; i++) row[i] = 1;
		break;
	}
	case 5: for (size_t i = 0; i < m; i++) { const unsigned r = rnd() % 6; row[i] = r < 3 ? 1 : r == 3 ? 0 : r == 4 ? 2 : (char)-1; } break; // other bytes
	default: for (size_t i = 0; i < m; i++) row[i] = (char)(rnd() & 1); break;      // random
	}
}

static void define_groups(Case &cs)
{
	cs.grp.assign(cs.W, std::vector<unsigned>(cs.m, NONE));
	cs.Kc.assign(cs.C, 0);
	for (unsigned c = 0; c < cs.C; c++) {
		const char *row = cs.sel.data() + (size_t)c * cs.m;
		size_t K = 0, k = 0;
		for (size_t i = 0; i < cs.m; i++) K += row[i] == 1;
		cs.Kc[c] = K;
		for (size_t i = 0; i < cs.m; i++)
			if (row[i] == 1) cs.grp[c][i] = (unsigned)((u64)k++ * cs.KM / std::max<size_t>(K, 1));
	}
	if (cs.with_main)
		for (size_t i = 0; i < cs.m; i++) cs.grp[cs.C][i] = (unsigned)std::min<u64>((u64)i * cs.KM / cs.m, cs.KM - 1);
}

// expected rows of the traces [lo, hi): sum and number of traces of (column, group)
static void expect_rows(const Case &cs, size_t lo, size_t hi, std::vector<u64> &sum, std::vector<size_t> &cnt)
{
	sum.assign((size_t)cs.W * cs.KM, 0); cnt.assign((size_t)cs.W * cs.KM, 0);
	for (unsigned c = 0; c < cs.W; c++)
		for (size_t i = lo; i < hi; i++)
			if (cs.grp[c][i] != NONE) { CHECK(cs.grp[c][i] < cs.KM); sum[(size_t)c * cs.KM + cs.grp[c][i]] += cs.x[i]; cnt[(size_t)c * cs.KM + cs.grp[c][i]]++; }
}

// row of (group, column) in the staged layout, as resample.hip's header comment states it: stage-major, column-major inside a stage
static unsigned staged_row(unsigned g, unsigned c, unsigned KM, unsigned W, unsigned gps)
{
	const unsigned s = g / gps, g0 = s * gps, ng = std::min(gps, KM - g0);
	return g0 * W + c * ng + (g - g0);
}

struct Tally { size_t cases = 0, direct = 0, snapshot = 0, snapshot_few = 0, two_seg = 0, multi_run_seg = 0, unwritten = 0, starts_in_run = 0, ends_in_run = 0, in_kept8 = 0, tiles = 0; } tally;

// the masked replicas of one ensemble (masked_tables.h) for the shard [first, first + len)
static void check_masked(const Case &cs, unsigned gps, bool allow_direct, size_t N, size_t first, size_t len)
{
	static MaskedPlan mp;
	static MaskedWork work;
	const unsigned W = cs.W, KM = cs.KM, nstage = (KM + gps - 1) / gps, nrow = KM * W;
	const bool direct = allow_direct && W <= 16;
	masked_build(mp, work, cs.m, cs.sel.data(), cs.C, KM, cs.with_main, gps, direct, masked_want_seg(N, 256), first, len);
	tally.cases++;
	CHECK(mp.W == W && mp.nstage == nstage && mp.direct == direct);
	// trace counts
	CHECK(mp.Kc.size() == cs.C && mp.Mv.size() == W);
	for (unsigned c = 0; c < cs.C; c++) CHECK(mp.Kc[c] == cs.Kc[c] && mp.Mv[c] == (double)cs.Kc[c]);
	if (cs.with_main) CHECK(mp.Mv[cs.C] == (double)cs.m);
	// the row map
	CHECK(mp.rowmap.size() == nrow);
	std::vector<char> seen(nrow, 0);
	for (unsigned c = 0; c < W; c++)
		for (unsigned g = 0; g < KM; g++) {
			const unsigned row = mp.rowmap[(size_t)c * KM + g];
			CHECK(row == staged_row(g, c, KM, W, gps) && row < nrow && !seen[row]);
			seen[row] = 1;
		}
	// runs: they tile the shard in order, none is empty, one signature in every column; a trace of a group of stage s lies in a run of a stage <= s
	const unsigned nr = (unsigned)mp.runs.size();
	CHECK(mp.stage_run0.size() == nstage + 1 && mp.stage_run0[nstage] == nr && (nr == 0 || mp.stage_run0[0] == 0));
	size_t t = 0;
	unsigned sg = 0;
	for (unsigned r = 0; r < nr; r++) {
		const Chunk &k = mp.runs[r];
		CHECK(k.t0 == t && k.count > 0 && t + k.count <= len);
		while (sg < nstage && r >= mp.stage_run0[sg + 1]) sg++;
		CHECK(sg < nstage && r >= mp.stage_run0[sg]);
		for (unsigned c = 0; c < W; c++)
			for (size_t i = 0; i < k.count; i++) {
				const unsigned g = cs.grp[c][first + t + i];
				CHECK(g == cs.grp[c][first + t]);
				CHECK(g == NONE || sg <= g / gps);
			}
		t += k.count;
	}
	CHECK(t == len);
	for (unsigned s = 0; s < nstage; s++) CHECK(mp.stage_run0[s] <= mp.stage_run0[s + 1]);
	std::vector<u64> want;
	std::vector<size_t> cnt;
	expect_rows(cs, first, first + len, want, cnt);
	bool some_empty = false;
	for (size_t n : cnt) some_empty |= n == 0;
	auto run_sum = [&](unsigned r) { u64 a = 0; for (size_t i = 0; i < mp.runs[r].count; i++) a += cs.x[first + mp.runs[r].t0 + i]; return a; };
	std::vector<u64> rows(nrow);
	std::vector<char> stored(nrow, 0);
	for (u64 &v : rows) v = rnd(); // (what the block held before)
	auto stage_rows_final = [&](unsigned s) { // the rows of the stage's groups are final when its walk is done
		for (unsigned g = s * gps; g < std::min(KM, (s + 1) * gps); g++)
			for (unsigned c = 0; c < W; c++)
				if (stored[mp.rowmap[(size_t)c * KM + g]] || (mp.direct && mp.unwritten)) CHECK(rows[mp.rowmap[(size_t)c * KM + g]] == want[(size_t)c * KM + g]);
	};
	if (mp.direct) {
		// k_rows_walk: a running sum per column; at the end of a run its sum goes to the member columns, a flushing column stores its sum and
		// starts over.  A stage in two segments: A starts from the carry, B from zero; k_seg_fix adds A's live sums to the first row B stored
		// (fix_row) or hands them on.  (masked_stream_stage, tspws_rows_walk_launch)
		tally.direct++;
		CHECK(mp.rdesc.size() == nr && mp.stage_mid.size() == nstage && mp.fix_row.size() == (size_t)nstage * W);
		CHECK(mp.unwritten == some_empty);
		tally.unwritten += mp.unwritten;
		if (mp.unwritten) std::fill(rows.begin(), rows.end(), 0);
		std::vector<u64> carry(W, 0);
		bool have_carry = false;
		size_t nflush = 0;
		for (unsigned s = 0; s < nstage; s++) {
			const unsigned q0 = mp.stage_run0[s], q1 = mp.stage_run0[s + 1];
			unsigned qm = mp.stage_mid[s];
			CHECK(qm >= q0 && qm <= q1);
			const bool two = qm < q1 && qm > q0;
			if (!two) qm = q1;
			std::vector<unsigned> first_in_b(W, NONE);
			if (q1 > q0) {
				std::vector<u64> endA(W, 0), endB(W, 0);
				for (int seg = 0; seg < (two ? 2 : 1); seg++) {
					std::vector<u64> P(W, 0);
					if (!seg && have_carry) P = carry;
					for (unsigned r = seg ? qm : q0; r < (seg ? q1 : qm); r++) {
						const RunDesc &d = mp.rdesc[r];
						CHECK(d.t0 == mp.runs[r].t0 && d.count == mp.runs[r].count && d.frow == nflush);
						if (W < 32) CHECK(!(d.member >> W) && !(d.flush >> W));
						CHECK(!(d.flush & ~d.member));
						const u64 a = run_sum(r);
						for (unsigned c = 0; c < W; c++) {
							if ((d.member >> c) & 1u) P[c] += a;
							if ((d.flush >> c) & 1u) {
								CHECK(nflush < mp.flush_rows.size());
								const unsigned row = mp.flush_rows[nflush++];
								CHECK(row < nrow && !stored[row]);
								rows[row] = P[c]; stored[row] = 1; P[c] = 0;
								if (seg && first_in_b[c] == NONE) first_in_b[c] = row;
							}
						}
					}
					(seg ? endB : endA) = P;
				}
				if (two) {
					tally.two_seg++;
					for (unsigned c = 0; c < W; c++) {
						const unsigned fr = mp.fix_row[(size_t)s * W + c];
						if (fr != NONE) { CHECK(fr < nrow); rows[fr] += endA[c]; carry[c] = endB[c]; }
						else carry[c] = endA[c] + endB[c];
					}
				} else carry = endA;
				have_carry = true;
			}
			for (unsigned c = 0; c < W; c++) CHECK(mp.fix_row[(size_t)s * W + c] == first_in_b[c]); // the first row c stores at or after stage_mid, else none
			stage_rows_final(s);
		}
		CHECK(nflush == mp.flush_rows.size());
	} else {
		// k_prefix_walk: a segment walks its runs without resetting its sum and stores a snapshot after every run; segment 0 of a stage starts
		// from the sum of the carry snapshots.  k_combine_terms: a row is the signed sum of its terms.  (masked_stream_stage)
		tally.snapshot++;
		tally.snapshot_few += W <= 16;
		CHECK(mp.rdesc.empty() && mp.flush_rows.empty());
		CHECK(mp.stage_seg0.size() == nstage + 1 && mp.carry_ptr.size() == nstage + 1 && mp.trow_ptr.size() == (size_t)nrow + 1 && mp.tidx.size() == mp.tcoef.size());
		CHECK(mp.stage_seg0[nstage] == mp.seg_first.size() && mp.carry_ptr[nstage] == mp.carry.size() && mp.trow_ptr[nrow] == mp.tidx.size());
		std::vector<u64> snap(nr);
		std::vector<char> snapped(nr, 0);
		for (unsigned s = 0; s < nstage; s++) {
			const unsigned k0 = mp.stage_seg0[s], nseg = mp.stage_seg0[s + 1] - k0 - 1;
			CHECK(mp.stage_seg0[s + 1] > k0 && mp.seg_first[k0] == mp.stage_run0[s] && mp.seg_first[k0 + nseg] == mp.stage_run0[s + 1]);
			u64 base = 0;
			for (unsigned k = mp.carry_ptr[s]; k < mp.carry_ptr[s + 1]; k++) { CHECK(mp.carry[k] < mp.stage_run0[s] && snapped[mp.carry[k]]); base += snap[mp.carry[k]]; }
			for (unsigned q = 0; q < nseg; q++) {
				const unsigned ra = mp.seg_first[k0 + q], rb = mp.seg_first[k0 + q + 1];
				CHECK(ra < rb); // (the launch has a workgroup per segment: none is idle)
				tally.multi_run_seg += rb - ra > 1;
				u64 acc = q ? 0 : base;
				for (unsigned r = ra; r < rb; r++) { acc += run_sum(r); snap[r] = acc; }
			}
			for (unsigned r = mp.stage_run0[s]; r < mp.stage_run0[s + 1]; r++) snapped[r] = 1;
			// the stage's rows [g0 W, (g0 + ng) W)
			const unsigned g0 = s * gps, r0 = g0 * W, r1 = r0 + std::min(gps, KM - g0) * W;
			for (unsigned row = r0; row < r1; row++) {
				u64 acc = 0;
				for (unsigned j = mp.trow_ptr[row]; j < mp.trow_ptr[row + 1]; j++) {
					CHECK(mp.tidx[j] < nr && snapped[mp.tidx[j]] && mp.tcoef[j] == (float)(long long)mp.tcoef[j] && mp.tcoef[j] != 0);
					acc += (u64)(long long)mp.tcoef[j] * snap[mp.tidx[j]];
				}
				rows[row] = acc; stored[row] = 1; // (k_combine_terms writes every row: one without terms becomes zero)
			}
			stage_rows_final(s);
		}
	}
	for (unsigned c = 0; c < W; c++)
		for (unsigned g = 0; g < KM; g++) {
			const unsigned row = mp.rowmap[(size_t)c * KM + g];
			if (mp.direct) CHECK((stored[row] != 0) == (cnt[(size_t)c * KM + g] != 0)); // never stored: exactly the rows without a trace
			CHECK(rows[row] == want[(size_t)c * KM + g]);
		}
	// the block: every array where its offset says, the 16-byte records on 16-byte offsets
	auto in_blob = [&](size_t off, const void *p, size_t bytes, size_t align) {
		CHECK(off % align == 0 && off + bytes <= mp.blob.size());
		CHECK(!bytes || !memcmp(mp.blob.data() + off, p, bytes));
	};
	if (!mp.direct) in_blob(0, mp.runs.data(), nr * sizeof(Chunk), 16);
	in_blob(mp.o_rd, mp.rdesc.data(), mp.rdesc.size() * sizeof(RunDesc), 16);
	in_blob(mp.o_mv, mp.Mv.data(), W * sizeof(double), 8);
	in_blob(mp.o_tp, mp.trow_ptr.data(), mp.trow_ptr.size() * 4, 4);
	in_blob(mp.o_ti, mp.tidx.data(), mp.tidx.size() * 4, 4);
	in_blob(mp.o_tc, mp.tcoef.data(), mp.tcoef.size() * 4, 4);
	in_blob(mp.o_map, mp.rowmap.data(), mp.rowmap.size() * 4, 4);
	in_blob(mp.o_seg, mp.seg_first.data(), mp.seg_first.size() * 4, 4);
	in_blob(mp.o_car, mp.carry.data(), mp.carry.size() * 4, 4);
	in_blob(mp.o_fr, mp.flush_rows.data(), mp.flush_rows.size() * 4, 4);
	in_blob(mp.o_fx, mp.fix_row.data(), mp.fix_row.size() * 4, 4);
	CHECK(!mp.blob.empty());
}

// the batch's walk (jk_batch_two_stage.hip: build_tile, k_jb2_rows_walk): the ensemble is columns [col0, col0 + m) of a wider selection and
// traces [f, f + m) of the batch; per tile of 16 columns the runs tile the ensemble, rows are column * KM + group
static void check_batch(const Case &cs)
{
	static ColumnWork work;
	const unsigned W = cs.W, KM = cs.KM, C = cs.C;
	const size_t m = cs.m, col0 = 3, Tn = m + 5, f = 11;
	std::vector<char> wide((size_t)C * Tn, 1);
	for (unsigned c = 0; c < C; c++) memcpy(wide.data() + (size_t)c * Tn + col0, cs.sel.data() + (size_t)c * m, m);
	std::vector<RunDesc> runs(2); // (other ensembles' tables in front)
	std::vector<unsigned> flush(5, 77), Kc(C, 99);
	std::vector<u64> want, rows((size_t)W * KM);
	std::vector<size_t> cnt;
	std::vector<char> stored((size_t)W * KM, 0);
	expect_rows(cs, 0, m, want, cnt);
	bool unwritten = false;
	size_t nflush = flush.size();
	for (unsigned c0 = 0; c0 < W; c0 += 16) {
		const unsigned c1 = std::min(W, c0 + 16);
		const size_t run0 = runs.size();
		auto sel = [&](unsigned c) { return c < C ? (const unsigned char *)wide.data() + (size_t)c * Tn + col0 : nullptr; };
		if (tile_runs(work, m, KM, c0, c1, sel, [&](unsigned g, unsigned c) { return c * KM + g; }, f, Kc.data(), runs, flush)) unwritten = true;
		tally.tiles++;
		std::vector<u64> P(16, 0);
		size_t t = 0;
		for (size_t r = run0; r < runs.size(); r++) {
			const RunDesc &d = runs[r];
			CHECK(d.t0 == f + t && d.count > 0 && t + d.count <= m && d.frow == nflush && !d.pad[0] && !d.pad[1]);
			CHECK(!(d.flush & ~d.member) && (c1 - c0 == 32 || !(d.member >> (c1 - c0))));
			u64 a = 0;
			for (size_t i = 0; i < d.count; i++) {
				a += cs.x[t + i];
				for (unsigned c = c0; c < c1; c++) CHECK(cs.grp[c][t + i] == cs.grp[c][t]);
			}
			for (unsigned c = c0; c < c1; c++) {
				if ((d.member >> (c - c0)) & 1u) P[c - c0] += a;
				if ((d.flush >> (c - c0)) & 1u) {
					CHECK(nflush < flush.size());
					const unsigned row = flush[nflush++];
					CHECK(row / KM == c && !stored[row]);
					rows[row] = P[c - c0]; stored[row] = 1; P[c - c0] = 0;
				}
			}
			t += d.count;
		}
		CHECK(t == m && nflush == flush.size());
	}
	bool some_empty = false;
	for (size_t k = 0; k < rows.size(); k++) {
		CHECK((stored[k] != 0) == (cnt[k] != 0));
		if (stored[k]) CHECK(rows[k] == want[k]);
		some_empty |= !cnt[k];
	}
	CHECK(unwritten == some_empty);
	for (unsigned c = 0; c < C; c++) CHECK(Kc[c] == cs.Kc[c]);
	for (unsigned k = 0; k < 5; k++) CHECK(flush[k] == 77);
}

int main()
{
	const size_t ms[] = {1, 2, 7, 8, 9, 63, 64, 65, 70, 257}, Ns[] = {1000, 4096, 87000}; // (87000 samples: three segments per stage)
	const unsigned Ws[] = {1, 15, 16, 17, 33};
	unsigned triple = 0, inner = 0;
	for (size_t m : ms)
		for (unsigned kq = 0; kq < 5; kq++)
			for (unsigned W : Ws) {
				Case cs;
				cs.m = m; cs.KM = kq == 0 ? 1 : kq == 1 ? 2 : kq == 2 ? 3 : kq == 3 ? 10 : (unsigned)m + 3; cs.W = W;
				cs.with_main = W > 1 && (triple & 1);
				cs.C = W - (cs.with_main ? 1 : 0);
				cs.sel.assign((size_t)cs.C * m, 0);
				for (unsigned c = 0; c < cs.C; c++) fill_column(cs.sel.data() + (size_t)c * m, m, cs.KM, c + triple, triple / 7 + c);
				cs.x.resize(m);
				for (u64 &v : cs.x) v = rnd();
				define_groups(cs);
				snprintf(case_text, sizeof case_text, "batch m=%zu KM=%u W=%u main=%d triple=%u", m, cs.KM, W, (int)cs.with_main, triple);
				check_batch(cs);
				const unsigned gpss[] = {1, 3, cs.KM};
				for (unsigned gps : gpss) {
					if (gps > cs.KM) continue;
					// shards: whole, empty, and three that start and end anywhere -- inside runs, inside kept stretches
					const size_t a = rnd() % m, b = rnd() % m;
					const size_t shard[5][2] = {{0, m}, {m / 2, 0}, {m / 3, m - m / 3 - m / 4}, {std::min(a, b), std::max(a, b) - std::min(a, b) + 1}, {m > 2 ? 1u : 0u, m > 2 ? m - 2 : m}};
					for (const auto &sh : shard) {
						const size_t first = sh[0], len = sh[1], N = Ns[(inner >> 1) % 3];
						const bool allow_direct = inner & 1;
						inner++;
						snprintf(case_text, sizeof case_text, "masked m=%zu KM=%u W=%u main=%d gps=%u direct=%d N=%zu shard=[%zu,+%zu) triple=%u", m, cs.KM, W, (int)cs.with_main, gps,
						         (int)allow_direct, N, first, len, triple);
						check_masked(cs, gps, allow_direct, N, first, len);
						// what the shards covered, by the definition: an edge inside a run (no column changes there), inside a stretch of >= 8 kept bytes
						auto same = [&](size_t i) { for (unsigned c = 0; c < W; c++) if (cs.grp[c][i - 1] != cs.grp[c][i]) return false; return true; };
						if (len && first > 0 && same(first)) tally.starts_in_run++;
						if (len && first + len < m && same(first + len)) tally.ends_in_run++;
						for (unsigned c = 0; c < cs.C && len; c++) {
							size_t lo = first, hi = first;
							const char *row = cs.sel.data() + (size_t)c * m;
							if (row[first] != 1 || !first || row[first - 1] != 1) continue;
							while (lo > 0 && row[lo - 1] == 1) lo--;
							while (hi < m && row[hi] == 1) hi++;
							if (hi - lo >= 8) { tally.in_kept8++; break; }
						}
					}
				}
				triple++;
			}
	// the grid reached every path
	CHECK(tally.direct > 500 && tally.snapshot > 500 && tally.snapshot_few > 100 && tally.two_seg > 100 && tally.multi_run_seg > 100 && tally.unwritten > 100);
	CHECK(tally.starts_in_run > 50 && tally.ends_in_run > 50 && tally.in_kept8 > 50 && tally.tiles > triple);
	printf("column_runs_check: %zu masked cases (%zu direct, %zu snapshot) and %u batch ensembles agree with the per-trace definition\n", tally.cases, tally.direct,
	       tally.snapshot, triple);
	return 0;
}
