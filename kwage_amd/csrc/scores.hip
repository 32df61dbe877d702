// kwage_amd/csrc/scores.hip -- kwage_search_scores (include/kwage_amd.h): the k-mer count of every column of a group
// for every query of a batch, as a dense queries x columns matrix of uint32 cells on the device.  No counterpart in
// the reference.
//
//   kmer_kernel  ->  score_tile_kernel
//               |->  count_kernel<SEG> + score_combine_kernel (long queries)
//
// The batch layout, the k-mer stage, the counter widths and the segment rule are engine.hip's (declared in
// engine_state.hpp), as are the host-side objects (context, group, batch); of kernels.hpp this unit instantiates
// count_kernel's SEG form and the device functions scores_kernels.hpp builds on.  No hit list, no atomic, no sort:
// each call writes queries x span x 4 bytes.
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

namespace kwage {
namespace {

thread_local char last_kernel[64] = "";

struct Events {
	hipEvent_t ev[2] = {nullptr, nullptr};
	~Events() { for(hipEvent_t e : ev){ if(e){ (void)hipEventDestroy(e); } } }
};

template <int PLANES, int NH>
void launch_tile(const SearchArgs &a, const ScoreArgs &sa, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a.n_queries*a.chunks;
	hipLaunchKernelGGL((score_tile_kernel<PLANES, NH>), dim3((uint32_t)((tiles + 3)/4)), dim3(SEARCH_THREADS), 0, s, a, sa);
}

template <int PLANES, int NH>
void launch_seg_count(const SearchArgs &a, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a.n_queries*a.segs*a.chunks;
	hipLaunchKernelGGL((count_kernel<PLANES, NH, true>), dim3((uint32_t)((tiles + 3)/4)), dim3(SEARCH_THREADS), 0, s, a);
}

template <int PLANES>
int launch_combine(const SearchArgs &a, const ScoreArgs &sa, uint32_t seg_planes, hipStream_t s)
{
	const size_t lds = (size_t)(COMBINE_WAVES/2)*PLANES*WAVE*16;
	static_assert((size_t)(COMBINE_WAVES/2)*WAVE >= (size_t)ScoreXch<PLANES>::LANES, "the epilogue's exchange fits the tree's LDS");
	if(lds > 48*1024){
		HIP_TRY(hipFuncSetAttribute((const void*)score_combine_kernel<PLANES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	}
	hipLaunchKernelGGL((score_combine_kernel<PLANES>), dim3(a.n_queries*a.chunks), dim3(COMBINE_WAVES*WAVE), lds, s, a, sa, seg_planes);
	return KWAGE_OK;
}

// dispatch on (planes, hash functions) as engine.hip's count path does
template <template <int, int> class F, typename... A>
void by_shape(uint32_t planes, uint32_t nh, A&&... args)
{
	auto go = [&](auto P) {
		constexpr int PL = decltype(P)::value;
		switch(nh){
			case 1: F<PL, 1>::run(args...); break;
			case 2: F<PL, 2>::run(args...); break;
			case 3: F<PL, 3>::run(args...); break;
			case 4: F<PL, 4>::run(args...); break;
			default: F<PL, 5>::run(args...); break;
		}
	};
	switch(planes){
		case 7: go(std::integral_constant<int, 7>()); break;
		case 10: go(std::integral_constant<int, 10>()); break;
		case 14: go(std::integral_constant<int, 14>()); break;
		case 20: go(std::integral_constant<int, 20>()); break;
		default: go(std::integral_constant<int, 32>()); break;
	}
}
template <int P, int NH> struct TileLaunch { static void run(const SearchArgs &a, const ScoreArgs &sa, hipStream_t s) { launch_tile<P, NH>(a, sa, s); } };
template <int P, int NH> struct SegLaunch { static void run(const SearchArgs &a, hipStream_t s) { launch_seg_count<P, NH>(a, s); } };

static const uint64_t SLAB_BYTES_PER_SLICE = 1ull << 30;       // partial counters of one slice of the queries (segmented form)

// Everything that can be refused without the device.
int scores_check(kwage_group *g, kwage_batch *b, uint64_t row_elems, const char *what)
{
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "kwage_group_finalize() must be called before searching"); }
	if(b->ctx != g->ctx){ return fail(KWAGE_ERR_ARG, "batch and group belong to different contexts"); }
	const uint64_t span = g->next_byte*8;
	if(row_elems < span || row_elems % 4 != 0){
		return fail(KWAGE_ERR_ARG, "%s: row_elems must be a multiple of 4 and at least the group's column span %llu (got %llu)", what,
		            (unsigned long long)span, (unsigned long long)row_elems);
	}
	return KWAGE_OK;
}

}  // namespace

// The launches' shapes, planned (and refused) before the first kernel.
int score_stage_plan(const kwage_group *g, uint32_t n, uint64_t max_count, ScorePlan *plan)
{
	kwage_ctx *ctx = g->ctx;
	const uint64_t span = g->next_byte*8;
	SearchArgs a;
	memset(&a, 0, sizeof(a));
	a.units_per_row = (uint32_t)(g->stride/16);
	a.chunks = (a.units_per_row + WAVE - 1)/WAVE;
	if((uint64_t)n*a.chunks > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
	uint32_t planes = 0, seg_planes = 0, slice = n;
	if(n && span){
		planes = planes_for(max_count);
		a.n_queries = n;
		choose_segments(a, max_count, 1024, ctx->tune.force_segs);
		seg_planes = (a.segs > 1) ? planes_for(a.seg_kmers) : planes;
		if(a.segs > 1){      // keep the slab of partial counters bounded: fewer queries per slice
			const uint64_t slab_per_q = (uint64_t)a.segs*seg_planes*g->stride;
			slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slice, SLAB_BYTES_PER_SLICE/slab_per_q));
			// score_combine_kernel's grid is one workgroup per (query, tile): a slice's threads stay below 2^32
			const uint64_t max_wgs = 0xFFFFFFFFull/(COMBINE_WAVES*WAVE);
			if(a.chunks > max_wgs){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
			slice = (uint32_t)std::min<uint64_t>(slice, max_wgs/a.chunks);
		}
		if((uint64_t)slice*a.segs*a.chunks/4 + 1 > 0x7FFFFFFFull){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
	}
	plan->units_per_row = a.units_per_row;
	plan->chunks = a.chunks;
	plan->planes = planes;
	plan->seg_planes = seg_planes;
	plan->segs = a.segs;
	plan->seg_kmers = a.seg_kmers;
	plan->slice = slice;
	return KWAGE_OK;
}

// ---- scores: tile kernels, or segments + combine slice by slice of the queries ---------------------------------------
int score_stage_run(kwage_group *g, const RowListView &v, const ScorePlan &plan, ScoreArgs sa, uint32_t flags, float *ms,
                    PoolBlocks &blocks, char *kernel_name)
{
	int rc;
	kwage_ctx *ctx = g->ctx;
	hipStream_t s = ctx->stream;
	const uint32_t n = v.n, nh = v.num_hash;
	const uint64_t span = g->next_byte*8;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0 && ms;
	Events ev;
	if(timing){ for(hipEvent_t &e : ev.ev){ HIP_TRY(hipEventCreate(&e)); } }
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[0], s)); }
	if(n && span){
		SearchArgs a;
		memset(&a, 0, sizeof(a));
		a.units_per_row = plan.units_per_row;
		a.chunks = plan.chunks;
		a.segs = plan.segs;
		a.seg_kmers = plan.seg_kmers;
		a.db = g->d_bits;
		a.stride = g->stride;
		a.valid = g->d_valid;
		a.rows = v.rows;
		a.num_hash = nh;
		const uint32_t planes = plan.planes, seg_planes = plan.seg_planes, slice = plan.slice;
		uint32_t *const out0 = sa.out;
		sa.span = span;
		sa.form = (ctx->tune.scores_form == (int64_t)SCORES_FORM_LANE) ? SCORES_FORM_LANE : SCORES_FORM_WAVE;
		if(a.segs > 1){
			uint32_t *slab = nullptr;
			if((rc = blocks.take((uint64_t)slice*a.segs*seg_planes*g->stride, &slab))){ return rc; }
			a.partial = slab;
			snprintf(kernel_name, 64, "count_kernel<%u,%u>+score_combine_kernel<%u>", seg_planes, std::min(nh, 5u), planes);
		}
		else{
			snprintf(kernel_name, 64, "score_tile_kernel<%u,%u>", planes, std::min(nh, 5u));
		}
		for(uint32_t q0 = 0; q0 < n; q0 += slice){
			a.n_queries = std::min(slice, n - q0);
			a.pos_off = v.pos_off + q0;
			a.nkmer = v.counts + q0;
			sa.out = out0 + (uint64_t)q0*sa.row_elems;
			if(a.segs > 1){
				by_shape<SegLaunch>(seg_planes, nh, a, s);
				HIP_TRY(hipGetLastError());
				switch(planes){
					case 7: rc = launch_combine<7>(a, sa, seg_planes, s); break;
					case 10: rc = launch_combine<10>(a, sa, seg_planes, s); break;
					case 14: rc = launch_combine<14>(a, sa, seg_planes, s); break;
					case 20: rc = launch_combine<20>(a, sa, seg_planes, s); break;
					default: rc = launch_combine<32>(a, sa, seg_planes, s); break;
				}
				if(rc){ return rc; }
			}
			else{
				by_shape<TileLaunch>(planes, nh, a, sa, s);
			}
			HIP_TRY(hipGetLastError());
		}
	}
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[1], s)); }
	HIP_TRY(hipStreamSynchronize(s));
	if(timing){ HIP_TRY(hipEventElapsedTime(ms, ev.ev[0], ev.ev[1])); }
	return KWAGE_OK;
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
	const uint32_t nh = g->params.num_hash;
	if(L->max_pos*nh > 0xFFFFFFFFull){
		return fail(KWAGE_ERR_ARG, "a query of %llu k-mer positions x %u hash functions exceeds 2^32 rows", (unsigned long long)L->max_pos, nh);
	}
	const uint32_t n = b->n;
	ScorePlan plan;
	if((rc = score_stage_plan(g, n, L->max_pos, &plan))){ return rc; }
	hipStream_t s = ctx->stream;

	uint32_t *d_rows = nullptr, *d_nkmer = nullptr, *d_qthr = nullptr;
	unsigned long long *d_tables = nullptr, *d_missing = nullptr;
	if((rc = blocks.take(std::max<uint64_t>(L->total_pos*nh, 1)*sizeof(uint32_t), &d_rows))){ return rc; }
	if((rc = blocks.take(std::max<uint64_t>(n, 1)*sizeof(uint32_t)*2 + 16, &d_nkmer))){ return rc; }
	d_qthr = d_nkmer + std::max<uint32_t>(n, 1);
	d_missing = (unsigned long long*)(((uintptr_t)(d_qthr + std::max<uint32_t>(n, 1)) + 7) & ~(uintptr_t)7);

	// ---- k-mer stage: distinct canonical k-mers and their row indices (threshold 0: every floor is 0) ------------------
	if(n){
		if(L->table_slots){
			if((rc = blocks.take(L->table_slots*sizeof(uint64_t), &d_tables))){ return rc; }
			HIP_TRY(hipMemsetAsync(d_tables, 0xFF, L->table_slots*sizeof(uint64_t), s));
		}
		const KmerStageOut o = {d_rows, nullptr, d_nkmer, d_qthr, d_tables};
		if((rc = launch_kmer_kernels(g->params, b, L, 0.0f, 0, o, s))){ return rc; }
		if(g->d_row_map){
			// a sparse group made for other queries is refused before a cell is written
			unsigned long long missing = 0;
			HIP_TRY(hipMemsetAsync(d_missing, 0, sizeof(unsigned long long), s));
			if((rc = launch_remap_rows(g, n, L, d_rows, d_nkmer, d_missing, s))){ return rc; }
			HIP_TRY(hipMemcpyAsync(&missing, d_missing, sizeof(missing), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			if(missing){
				return fail(KWAGE_ERR_STATE, "%llu row indices of this batch are not among the rows of the sparse group (it was created for other queries)", missing);
			}
		}
		// (the k-mer counts are final here: their copy is queued ahead of the score stage, which waits for the stream)
		if(num_query_kmer_dev){
			HIP_TRY(hipMemcpyAsync(num_query_kmer_dev, d_nkmer, (size_t)n*sizeof(uint32_t), hipMemcpyDefault, s));
		}
	}

	const RowListView v = {d_rows, L->d_pos_off, d_nkmer, n, L->max_pos, nh};
	ScoreArgs sa;
	sa.out = (uint32_t*)scores_dev;
	sa.row_elems = row_elems;
	sa.span = 0;
	sa.form = SCORES_FORM_WAVE;
	return score_stage_run(g, v, plan, sa, flags, search_kernel_ms, blocks, last_kernel);
}

// The host form: the matrix in a block of the context's pool (rows `span` cells apart), then one strided copy that
// leaves the caller's cells at or beyond the span alone.
int search_scores_host(kwage_group *g, kwage_batch *b, uint32_t *scores, uint64_t row_elems, uint32_t *num_query_kmer,
                       uint32_t flags, float *search_kernel_ms, PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_search_scores";
	const uint64_t span = g->next_byte*8;
	const uint32_t n = b->n;
	if((rc = scores_check(g, b, row_elems, what))){ return rc; }      // (on the caller's own row length, before anything is allocated)
	if(n && span && !scores){ return fail(KWAGE_ERR_ARG, "%s: scores is NULL", what); }
	if((rc = set_device(g->ctx))){ return rc; }
	uint32_t *d_scores = nullptr, *d_nk = nullptr;
	if((rc = blocks.take(std::max<uint64_t>((uint64_t)n*span, 4)*sizeof(uint32_t), &d_scores))){ return rc; }
	if(num_query_kmer && (rc = blocks.take(std::max<uint64_t>(n, 1)*sizeof(uint32_t), &d_nk))){ return rc; }
	if((rc = search_scores_device(g, b, d_scores, span, d_nk, flags, search_kernel_ms, blocks, what))){ return rc; }
	hipStream_t s = g->ctx->stream;
	if(n && span){
		HIP_TRY(hipMemcpy2DAsync(scores, row_elems*sizeof(uint32_t), d_scores, span*sizeof(uint32_t), span*sizeof(uint32_t), n,
		                         hipMemcpyDeviceToHost, s));
	}
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
	const int rc = kwage::search_scores_device(g, b, scores_dev, row_elems, num_query_kmer_dev, flags, search_kernel_ms, blocks,
	                                           "kwage_search_scores_device");
	if(rc){
		// an error return may leave kernels of this call queued: nothing of it may still run when `blocks` hands its
		// device memory back to the pool (its destructor, below)
		(void)hipStreamSynchronize(g->ctx->stream);
		(void)hipGetLastError();
	}
	return rc;
}

extern "C" int kwage_search_scores(kwage_group *g, kwage_batch *b, uint32_t *scores, uint64_t row_elems,
                                   uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms)
{
	if(!g || !b){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_scores: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	const int rc = kwage::search_scores_host(g, b, scores, row_elems, num_query_kmer, flags, search_kernel_ms, blocks);
	if(rc){      // as kwage_search_scores_device: nothing of this call may still run when `blocks` hands its memory back
		(void)hipStreamSynchronize(g->ctx->stream);
		(void)hipGetLastError();
	}
	return rc;
}

extern "C" const char *kwage_search_scores_kernel(void) { return kwage::last_kernel; }
