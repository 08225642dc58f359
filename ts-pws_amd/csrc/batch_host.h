// batch_host.h -- host code that the batched entry points share (batch.hip, jk_single.hip, jk_batch.hip, jk_batch_two_stage.hip, conv_batch.hip,
// sub_batch.hip, boot_batch.hip, weighted_batch.hip) and the row-analysis units: the lifetime of a call's uploads, the planning of finish batches, and
// the small loops over a selection that every unit needs.  Only what removes knowledge from its call sites lives here; the kernels they share are in
// batch_kernels.h, and what sub_batch.hip, boot_batch.hip and weighted_batch.hip share beyond that -- their kernels, round driver and argument check --
// in row_batch.h.  What needs no HIP runtime is in host_plan.h, which the CPU checks compile too: the layout of a table block (TableLayout), the
// rounds of whole ensembles (Round, whole_ensemble_rounds), participation and slots, task packing and the range checks.  coef_rows.h, on top of
// this header: the chunk and round drivers of the units that work on coefficient sets (wxs_rows.hip, ftan_rows.hip).
#pragma once

#include "tspws_internal.h"
#include "host_plan.h"

#include <deque>
#include <unordered_map>

// One batched call on one stream.  It owns the host blocks that are sources of hipMemcpyAsync: a copy from pageable memory may still read its
// source after hipMemcpyAsync has returned, so a source must outlive the stream work.  The entry point ends with a checked drain(); on every
// other way out the destructor waits for the stream before the blocks go, so no early return needs code of its own.
class BatchCall {
public:
	explicit BatchCall(hipStream_t st) : st_(st) {}
	BatchCall(const BatchCall &) = delete;
	~BatchCall() { if (!drained_) (void)hipStreamSynchronize(st_); }
	hipStream_t stream() const { return st_; }
	char *block(size_t bytes) { return blocks_.emplace_back(std::max<size_t>(bytes, 1), 0).data(); } // zeroed; alive until the call ends
	// the first `bytes` of a block of this call to the plan's scratch slot (at least `reserve` bytes of it: rounds that share a slot name their
	// largest table, so that the slot does not grow between them), stream-ordered; *dev = the device copy
	int upload(tspws_hip_plan *pl, int slot, const char *blk, size_t bytes, char **dev, size_t reserve = 0)
	{
		void *v;
		if (int rc = scratch(pl, slot, std::max<size_t>({bytes, reserve, 1}), &v)) return rc;
		HIP_TRY(hipMemcpyAsync(v, blk, bytes, hipMemcpyHostToDevice, st_));
		*dev = (char *)v;
		return 0;
	}
	// the call's last step: everything enqueued is complete (or has failed: the error is the caller's to report)
	hipError_t drain() { drained_ = true; return hipStreamSynchronize(st_); }

private:
	hipStream_t st_;
	bool drained_ = false;
	std::deque<std::vector<char>> blocks_;
};

// an argument refused: "who: what" (what: the message tail that a check of the host plans returns)
static inline int refuse(const char *who, const char *what) { return fail(TSPWS_E_ARG, (std::string(who) + ": " + what).c_str()); }

// Rows of one finish batch: sets, reconstructions and the inverse's octave buffer of the batch within `budget` at per_row bytes a row
// (tspws_inverse_row_bytes, times whatever shares the batch); even, so that the inverse pairs the same rows whatever the batching; at most
// 65534 (grid.y of the epilogues) and `cap`
static inline size_t even_rows_per_batch(size_t budget, size_t per_row, size_t cap)
{
	return std::min<size_t>({cap, 65534, std::max<size_t>(2, (budget / per_row) & ~(size_t)1)});
}

// kept traces of one row of a selection (bytes == 1)
static inline unsigned kept_count(const char *row, size_t m)
{
	unsigned k = 0;
	for (size_t i = 0; i < m; i++) k += row[i] == 1;
	return k;
}

// columns [col0, col0 + m) of sel[C][T] as a contiguous [C][m] block of the call: the selection of one ensemble for the single calls
static inline const char *ensemble_selection(BatchCall &call, const char *sel, unsigned C, size_t T, size_t col0, size_t m)
{
	char *out = call.block((size_t)C * m);
	for (unsigned c = 0; c < C; c++) memcpy(out + (size_t)c * m, sel + (size_t)c * T + col0, m);
	return out;
}

// classes of the columns [col0, col0 + m) of sel[C][T]: identical columns, numbered in order of first appearance; cls[i] = class of column
// col0 + i, first[k] = first column (relative to col0) of class k
static inline void selection_classes_strided(const char *sel, unsigned C, size_t T, size_t col0, size_t m, unsigned *cls, std::vector<size_t> &first)
{
	const size_t nbytes = ((size_t)C + 7) / 8;
	std::unordered_map<std::string, unsigned> id;
	std::string key(nbytes, '\0');
	first.clear();
	for (size_t i = 0; i < m; i++) {
		std::fill(key.begin(), key.end(), '\0');
		for (unsigned c = 0; c < C; c++)
			if (sel[(size_t)c * T + col0 + i] == 1) key[c >> 3] = (char)(key[c >> 3] | (1 << (c & 7)));
		auto it = id.find(key);
		if (it == id.end()) { it = id.emplace(key, (unsigned)first.size()).first; first.push_back(i); }
		cls[i] = it->second;
	}
}

// zero rows for the ensembles without traces: per output (base, floats per ensemble; a NULL base is skipped) the block of every empty ensemble
static inline int zero_empty_ensembles(const size_t *h_first, unsigned B, hipStream_t st, std::initializer_list<std::pair<float *, size_t>> outs)
{
	for (unsigned b = 0; b < B; b++)
		if (h_first[b + 1] == h_first[b])
			for (const auto &o : outs)
				if (o.first) HIP_TRY(hipMemsetAsync(o.first + (size_t)b * o.second, 0, o.second * sizeof(float), st));
	return 0;
}
