// kwage_amd/csrc/score_stage.hpp -- the score stage of the dense searches, shared by scores.hip (which defines it and
// owns its kernels) and filterset.hip (which hands it row lists that no k-mer stage made).  The stage counts, for
// every list of a row-list view, in how many of the list's rows each column of a group is set, and writes the counts
// as one row of uint32 cells: kwage_search_scores' matrix.
#ifndef KWAGE_AMD_SCORE_STAGE_HPP
#define KWAGE_AMD_SCORE_STAGE_HPP

#include <stdint.h>

#include "engine_state.hpp"
#include "pool_blocks.hpp"

namespace kwage {

static constexpr uint32_t SCORES_FORM_WAVE = 0, SCORES_FORM_LANE = 1;

struct ScoreArgs {
	uint32_t *out;                  // cell (q, c) of the launch's queries at out[q*row_elems + c]
	unsigned long long row_elems;   // cells between rows (multiple of 4, >= span)
	unsigned long long span;        // columns of the group (multiple of 8): cells at or beyond it are never written
	uint32_t form;                  // SCORES_FORM_*
};

// n row lists on the device, the shape SearchArgs::rows / pos_off / nkmer have: list i is the counts[i] entries
// [num_hash row indices each] from rows[pos_off[i]*num_hash] on.  max_count: the longest list (it picks the counters'
// width).  Every row index addresses a row of the group the view is searched in.
struct RowListView {
	const uint32_t *rows;
	const uint64_t *pos_off;        // n + 1
	const uint32_t *counts;         // n
	uint32_t n;
	uint64_t max_count;
	uint32_t num_hash;
};

// The launches' shapes: planned, and refused, on the host.
struct ScorePlan {
	uint32_t units_per_row, chunks;
	uint32_t planes, seg_planes;    // counter widths of the whole list and of one segment
	uint32_t segs, seg_kmers;
	uint32_t slice;                 // lists per launch (the segmented form keeps its slab of partial counters bounded)
};

// Everything about the launches that can be refused without the device (KWAGE_ERR_ARG: too large for one launch).
int score_stage_plan(const kwage_group *g, uint32_t n, uint64_t max_count, ScorePlan *plan);

// The stage itself on the context's first stream, waited for: the tile kernels, or segments + combine slice by slice
// of the lists.  sa: out / row_elems of list 0 (span and form are filled in here).  kernel_name (64 bytes) receives
// the kernels' names; with KWAGE_SEARCH_TIMING in flags and ms != NULL, *ms the HIP-event duration of the launches.
int score_stage_run(kwage_group *g, const RowListView &v, const ScorePlan &plan, ScoreArgs sa, uint32_t flags, float *ms,
                    PoolBlocks &blocks, char *kernel_name);

}  // namespace kwage

#endif
