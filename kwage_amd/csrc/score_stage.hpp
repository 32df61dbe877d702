// kwage_amd/csrc/score_stage.hpp -- the score stage of the dense searches, shared by scores.hip (which defines it and
// owns its kernels) and filterset.hip (which hands it row lists that no k-mer stage made).  The stage counts, for
// every list of a row-list view, in how many of the list's rows each column of a group is set, and writes the counts
// as one row of uint32 cells: kwage_search_scores' matrix.  The row-list view and the plan are engine_state.hpp's (the
// top-k search shares them); the launches are tile_search.hpp's, which only scores.hip of the two includes.
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

// Everything about the launches that can be refused without the device (KWAGE_ERR_ARG: too large for one launch).
int score_stage_plan(const kwage_group *g, uint32_t n, uint64_t max_count, TilePlan *plan);

// The stage itself on the context's first stream, waited for: the tile kernels, or segments + combine slice by slice
// of the lists.  sa: out / row_elems of list 0 (span and form are filled in here).  kernel_name (64 bytes) receives
// the kernels' names; with KWAGE_SEARCH_TIMING in flags and ms != NULL, *ms the HIP-event duration of the launches.
int score_stage_run(kwage_group *g, const RowListView &v, const TilePlan &plan, ScoreArgs sa, uint32_t flags, float *ms,
                    PoolBlocks &blocks, char *kernel_name);

// The host form of a dense search: the matrix in a block of the call (rows `span` cells apart), filled and waited for
// by device_form(d_scores, span), then one strided copy -- queued on the context's first stream, not waited for -- that
// leaves the caller's cells at or beyond the span alone.
template <typename F>
int scores_to_host(kwage_group *g, uint32_t n, uint32_t *scores, uint64_t row_elems, PoolBlocks &blocks, const char *what, F &&device_form)
{
	int rc;
	const uint64_t span = g->next_byte*8;
	if(n && span && !scores){ return fail(KWAGE_ERR_ARG, "%s: scores is NULL", what); }
	if((rc = set_device(g->ctx))){ return rc; }
	uint32_t *d_scores = nullptr;
	if((rc = blocks.take(std::max<uint64_t>((uint64_t)n*span, 4)*sizeof(uint32_t), &d_scores))){ return rc; }
	if((rc = device_form(d_scores, span))){ return rc; }
	if(n && span){
		HIP_TRY(hipMemcpy2DAsync(scores, row_elems*sizeof(uint32_t), d_scores, span*sizeof(uint32_t), span*sizeof(uint32_t), n,
		                         hipMemcpyDeviceToHost, g->ctx->stream));
	}
	return KWAGE_OK;
}

}  // namespace kwage

#endif
