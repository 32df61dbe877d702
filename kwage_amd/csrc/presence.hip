// kwage_amd/csrc/presence.hip -- kwage_search_presence (include/kwage_amd.h): for every query of a batch the bit vector
// of the columns of a group that pass the threshold, as a queries x row-bytes bitmap on the device -- bit (q, c) is set
// exactly where kwage_search at the same threshold reports a record.  What a BIGSI-style index answers natively.
//
//   kmer_kernel  ->  presence_tile_kernel
//               |->  count_kernel<SEG> + presence_combine_kernel (few long queries)
//               |->  presence_and_kernel (t = 1, unsegmented)
//               `->  presence_popcount_kernel (only where the rows' bit counts are asked for)
//
// The batch layout, the k-mer stage, the counter widths and the segment rule are engine.hip's (declared in
// engine_state.hpp); the k-mer stage into blocks of the call is pool_blocks.hpp's, the launches and the slice driver of
// the counted forms are tile_search.hpp's (shared with topk.hip and scores.hip).  Of kernels.hpp this unit instantiates
// count_kernel's SEG form and the device functions presence_kernels.hpp builds on.  No hit list, no atomic, no sort, no
// regrowth: each call writes queries x W bytes, W = the group's row bytes rounded up to 16.
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
#include "kernels.hpp"
#include "presence_kernels.hpp"
#include "tile_search.hpp"

namespace kwage {
namespace {

thread_local char last_kernel[64] = "";

struct PresenceKernels {
	using Epi = PresenceArgs;
	static constexpr const char *tile_name = "presence_tile_kernel<%u,%u>";
	static constexpr const char *seg_name = "count_kernel<%u,%u>+presence_combine_kernel<%u>";
	template <int PLANES, int NH> static auto tile() { return presence_tile_kernel<PLANES, NH>; }
	template <int PLANES> static auto combine() { return presence_combine_kernel<PLANES>; }
};

// bytes of a row of the bitmap that a search writes
uint64_t written_bytes(const kwage_group *g) { return (g->next_byte + 15)/16*16; }

// Everything that can be refused without the device.
int presence_check(kwage_group *g, kwage_batch *b, float threshold, uint64_t row_bytes, const char *what)
{
	int rc;
	if((rc = search_check(g, b))){ return rc; }
	if(!(threshold >= 0.0f && threshold <= 1.0f)){ return fail(KWAGE_ERR_ARG, "%s: threshold must satisfy 0 <= t <= 1", what); }
	const uint64_t w = written_bytes(g);
	if(row_bytes < w || row_bytes % 16 != 0){
		return fail(KWAGE_ERR_ARG, "%s: row_bytes must be a multiple of 16 and at least the group's row bytes rounded up to 16, %llu (got %llu)", what,
		            (unsigned long long)w, (unsigned long long)row_bytes);
	}
	return KWAGE_OK;
}

// presence_and_kernel over the plan's slices of the queries (the plan is unsegmented); after_slice as run_tile_slices'.
template <typename After>
int run_and_slices(const kwage_group *g, const RowListView &v, const TilePlan &plan, const PresenceArgs &e, char *kernel_name, hipStream_t s,
                   After &&after_slice)
{
	int rc;
	SearchArgs a;
	memset(&a, 0, sizeof(a));
	a.db = g->d_bits;
	a.stride = g->stride;
	a.units_per_row = plan.units_per_row;
	a.valid = g->d_valid;
	a.rows = v.rows;
	a.num_hash = v.num_hash;
	a.chunks = plan.chunks;
	a.segs = 1;
	snprintf(kernel_name, 64, "presence_and_kernel");
	for(uint32_t q0 = 0; q0 < v.n; q0 += plan.slice){
		a.n_queries = std::min(plan.slice, v.n - q0);
		a.pos_off = v.pos_off + q0;
		a.nkmer = v.counts + q0;
		const uint64_t tiles = (uint64_t)a.n_queries*a.chunks;
		hipLaunchKernelGGL(presence_and_kernel, dim3((uint32_t)((tiles + 3)/4)), dim3(SEARCH_THREADS), 0, s, a, e);
		HIP_TRY(hipGetLastError());
		if((rc = after_slice(a, q0))){ return rc; }
	}
	return KWAGE_OK;
}

// The whole search, queued on the context's first stream and waited for.
int search_presence_device(kwage_group *g, kwage_batch *b, float threshold, void *bits_dev, uint64_t row_bytes, void *passing_dev,
                           void *num_query_kmer_dev, uint32_t flags, float *search_kernel_ms, PoolBlocks &blocks, const char *what)
{
	int rc;
	last_kernel[0] = 0;
	if(search_kernel_ms){ *search_kernel_ms = 0; }
	if((rc = presence_check(g, b, threshold, row_bytes, what))){ return rc; }
	if(b->n && g->next_byte && (!bits_dev || ((uintptr_t)bits_dev & 15u))){
		return fail(KWAGE_ERR_ARG, "%s: the bitmap must be a 16-byte aligned device pointer", what);
	}
	kwage_ctx *ctx = g->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const KmerLayout *L = nullptr;
	if((rc = batch_prepare(b, g->params.kmer_len, &L))){ return rc; }
	const uint32_t n = b->n;
	const bool any = n && g->next_byte;
	// the launches' shapes; presence_combine_kernel's grid is one workgroup per (query, tile): a slice's threads stay below 2^32
	TilePlan plan;
	if((rc = plan_tiles(g, L->max_pos, any ? n : 0, 0xFFFFFFFFull/(COMBINE_WAVES*WAVE), &plan))){ return rc; }
	if((uint64_t)n*plan.chunks > 0xFFFFFFFFull || (passing_dev && n > 0x7FFFFFFFull)){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
	hipStream_t s = ctx->stream;

	// ---- k-mer stage: distinct canonical k-mers, their row indices, the floor (unsigned)(t * n) of every query ---------
	KmerBlocks kb;
	if((rc = kmer_prologue_checked(g, b, L, threshold, num_query_kmer_dev, blocks, s, &kb))){ return rc; }

	// ---- presence: tile kernels, the AND kernel, or segments + combine, slice by slice of the queries -------------------
	return timed_section((flags & KWAGE_SEARCH_TIMING) != 0 && search_kernel_ms, s, search_kernel_ms, [&]() -> int {
		PresenceArgs pa;
		pa.out = (uint8_t*)bits_dev;
		pa.row_bytes = row_bytes;
		pa.w_units = (uint32_t)(written_bytes(g)/16);
		pa.early_exit = (flags & KWAGE_SEARCH_EARLY_EXIT) ? 1 : 0;
		if(!any){
			if(n && passing_dev){ HIP_TRY(hipMemsetAsync(passing_dev, 0, (size_t)n*sizeof(uint32_t), s)); }      // (a group without columns)
			return KWAGE_OK;
		}
		const RowListView v = {kb.rows, L->d_pos_off, kb.nkmer, n, L->max_pos, g->params.num_hash};
		PresenceArgs slice_pa = pa;
		const auto next_slice = [&](const SearchArgs &a, uint32_t) -> int {
			slice_pa.out += (uint64_t)a.n_queries*row_bytes;
			return KWAGE_OK;
		};
		if(threshold == 1.0f && plan.segs == 1){ rc = run_and_slices(g, v, plan, slice_pa, last_kernel, s, next_slice); }
		else{ rc = run_tile_slices<PresenceKernels>(g, v, kb.qthr, plan, slice_pa, blocks, last_kernel, s, next_slice); }
		if(rc){ return rc; }
		if(passing_dev){
			hipLaunchKernelGGL(presence_popcount_kernel, dim3(n), dim3(POPCOUNT_THREADS), 0, s, pa, (uint32_t*)passing_dev);
			HIP_TRY(hipGetLastError());
		}
		return KWAGE_OK;
	});
}

// The host form: the bitmap in a block of the call (rows W bytes apart), then one strided copy that leaves the caller's
// bytes at or beyond W alone (the pattern of score_stage.hpp's scores_to_host); the per-query words through a block of
// their own.
int search_presence_host(kwage_group *g, kwage_batch *b, float threshold, uint8_t *bits, uint64_t row_bytes, uint32_t *passing,
                         uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms, PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_search_presence";
	const uint32_t n = b->n, n1 = std::max<uint32_t>(n, 1);
	if((rc = presence_check(g, b, threshold, row_bytes, what))){ return rc; }      // (on the caller's own row length, before anything is allocated)
	const uint64_t w = written_bytes(g);
	if(n && w && !bits){ return fail(KWAGE_ERR_ARG, "%s: bits is NULL", what); }
	if((rc = set_device(g->ctx))){ return rc; }
	uint8_t *d_bits = nullptr;
	uint32_t *d_words = nullptr;
	if((rc = blocks.take(std::max<uint64_t>((uint64_t)n*w, 16), &d_bits))){ return rc; }
	if((rc = blocks.take((uint64_t)n1*2*sizeof(uint32_t), &d_words))){ return rc; }
	uint32_t *d_passing = passing ? d_words : nullptr, *d_nk = num_query_kmer ? d_words + n1 : nullptr;
	if((rc = search_presence_device(g, b, threshold, d_bits, w, d_passing, d_nk, flags, search_kernel_ms, blocks, what))){ return rc; }
	hipStream_t s = g->ctx->stream;
	if(n && w){ HIP_TRY(hipMemcpy2DAsync(bits, row_bytes, d_bits, w, w, n, hipMemcpyDeviceToHost, s)); }
	if(passing && n){ HIP_TRY(hipMemcpyAsync(passing, d_passing, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s)); }
	if(num_query_kmer && n){ HIP_TRY(hipMemcpyAsync(num_query_kmer, d_nk, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s)); }
	HIP_TRY(hipStreamSynchronize(s));
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_search_presence_device(kwage_group *g, kwage_batch *b, float threshold, void *bits_dev, uint64_t row_bytes,
                                            void *passing_dev, void *num_query_kmer_dev, uint32_t flags, float *search_kernel_ms)
{
	if(!g || !b){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_presence_device: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_presence_device(g, b, threshold, bits_dev, row_bytes, passing_dev, num_query_kmer_dev, flags,
	                                                           search_kernel_ms, blocks, "kwage_search_presence_device"));
}

extern "C" int kwage_search_presence(kwage_group *g, kwage_batch *b, float threshold, uint8_t *bits, uint64_t row_bytes,
                                     uint32_t *passing, uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms)
{
	if(!g || !b){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_presence: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_presence_host(g, b, threshold, bits, row_bytes, passing, num_query_kmer, flags, search_kernel_ms, blocks));
}

extern "C" const char *kwage_search_presence_kernel(void) { return kwage::last_kernel; }
