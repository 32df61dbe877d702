// kwage_amd/csrc/scores.hip -- kwage_search_scores (include/kwage_amd.h): the k-mer count of every column of a group
// for every query of a batch, as a dense queries x columns matrix of uint32 cells on the device.  No counterpart in
// the reference.
//
//   kmer_kernel  ->  score_tile_kernel
//               |->  count_kernel<SEG> + score_combine_kernel (long queries)
//
// The batch layout, the k-mer stage, the counter widths and the segment rule are engine.hip's (declared in
// engine_state.hpp), as are the host-side objects (context, group, batch); the k-mer stage into blocks of the call is
// pool_blocks.hpp's, the launches and the slice driver are tile_search.hpp's (shared with topk.hip).  Of kernels.hpp this
// unit instantiates count_kernel's SEG form and the device functions scores_kernels.hpp builds on.  No hit list, no
// atomic, no sort: each call writes queries x span x 4 bytes.
//
// The score stage (score_stage.hpp: score_stage_plan, score_stage_run) takes a row-list view, not a batch: the filter
// search (filterset.hip) runs it over row lists that no k-mer stage made.  Every score kernel lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kwage_amd.h"
#include "engine_state.hpp"
#include "pool_blocks.hpp"
#include "score_stage.hpp"
#include "kernels.hpp"
#include "scores_kernels.hpp"
#include "tile_search.hpp"

namespace kwage {
namespace {

thread_local char last_kernel[64] = "";

struct ScoreKernels {
	using Epi = ScoreArgs;
	static constexpr const char *tile_name = "score_tile_kernel<%u,%u>";
	static constexpr const char *seg_name = "count_kernel<%u,%u>+score_combine_kernel<%u>";
	template <int PLANES, int NH> static auto tile() { return score_tile_kernel<PLANES, NH>; }
	template <int PLANES> static auto combine()
	{
		static_assert((size_t)(COMBINE_WAVES/2)*WAVE >= (size_t)ScoreXch<PLANES>::LANES, "the epilogue's exchange fits the tree's LDS");
		return score_combine_kernel<PLANES>;
	}
};

// Everything that can be refused without the device.
int scores_check(kwage_group *g, kwage_batch *b, uint64_t row_elems, const char *what)
{
	int rc;
	if((rc = search_check(g, b))){ return rc; }
	const uint64_t span = g->next_byte*8;
	if(row_elems < span || row_elems % 4 != 0){
		return fail(KWAGE_ERR_ARG, "%s: row_elems must be a multiple of 4 and at least the group's column span %llu (got %llu)", what,
		            (unsigned long long)span, (unsigned long long)row_elems);
	}
	return KWAGE_OK;
}

}  // namespace

// The launches' shapes, planned (and refused) before the first kernel.
int score_stage_plan(const kwage_group *g, uint32_t n, uint64_t max_count, TilePlan *plan)
{
	int rc;
	// score_combine_kernel's grid is one workgroup per (query, tile): a slice's threads stay below 2^32
	if((rc = plan_tiles(g, max_count, g->next_byte ? n : 0, 0xFFFFFFFFull/(COMBINE_WAVES*WAVE), plan))){ return rc; }
	if((uint64_t)n*plan->chunks > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
	return KWAGE_OK;
}

// ---- scores: tile kernels, or segments + combine slice by slice of the queries ---------------------------------------
int score_stage_run(kwage_group *g, const RowListView &v, const TilePlan &plan, ScoreArgs sa, uint32_t flags, float *ms,
                    PoolBlocks &blocks, char *kernel_name)
{
	kwage_ctx *ctx = g->ctx;
	hipStream_t s = ctx->stream;
	const uint64_t span = g->next_byte*8;
	return timed_section((flags & KWAGE_SEARCH_TIMING) != 0 && ms, s, ms, [&]() -> int {
		if(!v.n || !span){ return KWAGE_OK; }
		sa.span = span;
		sa.form = (ctx->tune.scores_form == (int64_t)SCORES_FORM_LANE) ? SCORES_FORM_LANE : SCORES_FORM_WAVE;
		return run_tile_slices<ScoreKernels>(g, v, nullptr, plan, sa, blocks, kernel_name, s, [&](const SearchArgs &a, uint32_t) -> int {
			sa.out += (uint64_t)a.n_queries*sa.row_elems;
			return KWAGE_OK;
		});
	});
}

namespace {

// The whole search, queued on the context's first stream and waited for.
int search_scores_device(kwage_group *g, kwage_batch *b, void *scores_dev, uint64_t row_elems, void *num_query_kmer_dev,
                         uint32_t flags, float *search_kernel_ms, PoolBlocks &blocks, const char *what)
{
	int rc;
	last_kernel[0] = 0;
	if(search_kernel_ms){ *search_kernel_ms = 0; }
	if((rc = scores_check(g, b, row_elems, what))){ return rc; }
	if(b->n && g->next_byte && (!scores_dev || ((uintptr_t)scores_dev & 15u))){
		return fail(KWAGE_ERR_ARG, "%s: the score matrix must be a 16-byte aligned device pointer", what);
	}
	kwage_ctx *ctx = g->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const KmerLayout *L = nullptr;
	if((rc = batch_prepare(b, g->params.kmer_len, &L))){ return rc; }
	const uint32_t n = b->n;
	TilePlan plan;
	if((rc = score_stage_plan(g, n, L->max_pos, &plan))){ return rc; }
	hipStream_t s = ctx->stream;

	// ---- k-mer stage: distinct canonical k-mers and their row indices (threshold 0: every floor is 0) ------------------
	KmerBlocks kb;
	if((rc = kmer_prologue_checked(g, b, L, 0.0f, num_query_kmer_dev, blocks, s, &kb))){ return rc; }

	const RowListView v = {kb.rows, L->d_pos_off, kb.nkmer, n, L->max_pos, g->params.num_hash};
	ScoreArgs sa;
	sa.out = (uint32_t*)scores_dev;
	sa.row_elems = row_elems;
	sa.span = 0;
	sa.form = SCORES_FORM_WAVE;
	return score_stage_run(g, v, plan, sa, flags, search_kernel_ms, blocks, last_kernel);
}

// The host form (score_stage.hpp scores_to_host), with the k-mer counts through a block of their own.
int search_scores_host(kwage_group *g, kwage_batch *b, uint32_t *scores, uint64_t row_elems, uint32_t *num_query_kmer,
                       uint32_t flags, float *search_kernel_ms, PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_search_scores";
	const uint32_t n = b->n;
	if((rc = scores_check(g, b, row_elems, what))){ return rc; }      // (on the caller's own row length, before anything is allocated)
	uint32_t *d_nk = nullptr;
	rc = scores_to_host(g, n, scores, row_elems, blocks, what, [&](uint32_t *d_scores, uint64_t span) -> int {
		int rc;
		if(num_query_kmer && (rc = blocks.take(std::max<uint64_t>(n, 1)*sizeof(uint32_t), &d_nk))){ return rc; }
		return search_scores_device(g, b, d_scores, span, d_nk, flags, search_kernel_ms, blocks, what);
	});
	if(rc){ return rc; }
	hipStream_t s = g->ctx->stream;
	if(num_query_kmer && n){ HIP_TRY(hipMemcpyAsync(num_query_kmer, d_nk, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s)); }
	HIP_TRY(hipStreamSynchronize(s));
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_search_scores_device(kwage_group *g, kwage_batch *b, void *scores_dev, uint64_t row_elems,
                                          void *num_query_kmer_dev, uint32_t flags, float *search_kernel_ms)
{
	if(!g || !b){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_scores_device: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_scores_device(g, b, scores_dev, row_elems, num_query_kmer_dev, flags, search_kernel_ms, blocks,
	                                                         "kwage_search_scores_device"));
}

extern "C" int kwage_search_scores(kwage_group *g, kwage_batch *b, uint32_t *scores, uint64_t row_elems,
                                   uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms)
{
	if(!g || !b){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_scores: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_scores_host(g, b, scores, row_elems, num_query_kmer, flags, search_kernel_ms, blocks));
}

extern "C" const char *kwage_search_scores_kernel(void) { return kwage::last_kernel; }
