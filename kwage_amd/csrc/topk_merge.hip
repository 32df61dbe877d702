// kwage_amd/csrc/topk_merge.hip -- kwage_topk_merge_device (include/kwage_amd.h): top-k lists of several shards, groups
// or passes merged on the device to the first k records per query under (num_match descending, order[column]
// ascending).  What a sharded top-k search runs on every rank that holds several units, and on rank 0 once per exchange.
//
//   merge_count_kernel -> merge_scan_kernel -> merge_scatter_kernel -> merge_select_kernel    (topk_merge_kernels.hpp)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "kwage_amd.h"
#include "engine_state.hpp"
#include "pool_blocks.hpp"
#include "topk_merge_kernels.hpp"

namespace kwage {
namespace {

static const uint32_t STREAM_BLOCKS_MAX = 4096;     // grid of the two passes over the records (grid-stride loops)
static const uint32_t SELECT_BLOCKS_MAX = 1u << 20;  // grid of the select kernel (it loops over the queries beyond)

// Buckets of at most this many records on average go to the one-wave form of the select kernel (KWAGE_TOPK_MERGE_WAVE
// overrides: 0 = always a workgroup of 256, 1 = always one wave).
uint32_t select_block(uint64_t n_hits, uint32_t n_queries, uint32_t k)
{
	static const int force = [] { const char *e = getenv("KWAGE_TOPK_MERGE_WAVE"); return e ? atoi(e) : -1; }();
	if(force == 0){ return 256; }
	if(force == 1){ return TM_WAVE; }
	return (k <= 64 && n_hits <= (uint64_t)n_queries*256) ? TM_WAVE : 256;
}

int topk_merge(kwage_ctx *ctx, const void *hits_dev, uint64_t n_hits, uint32_t n_queries, uint32_t k, const void *order_dev,
               uint64_t n_order, void *out_dev, uint64_t out_capacity, void *out_count_dev, PoolBlocks &blocks)
{
	int rc;
	if(k < 1 || k > KWAGE_TOPK_MAX){ return fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: k must satisfy 1 <= k <= %u (got %u)", (unsigned)KWAGE_TOPK_MAX, k); }
	if(n_hits > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: %llu records (at most 2^32 - 1)", (unsigned long long)n_hits); }
	if(n_queries > 0x7FFFFFFFu){ return fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: %u queries (at most 2^31 - 1)", n_queries); }
	if((rc = set_device(ctx))){ return rc; }
	hipStream_t s = ctx->stream;
	MergeArgs a;
	a.hits = (const kwage_hit*)hits_dev;
	a.n_hits = n_hits;
	a.n_queries = n_queries;
	a.k = k;
	a.order = (const uint32_t*)order_dev;
	a.n_order = n_order;
	a.out = (kwage_hit*)out_dev;
	a.out_capacity = out_capacity;
	a.out_count = (unsigned long long*)out_count_dev;
	const uint64_t nq = n_queries;
	// one block for the counters: bad (8 B), bucket_n, bucket_off, out_off
	unsigned long long *tables = nullptr;
	const uint64_t words = 1 + (nq + 1)/2 + (nq + 2)/2 + (nq + 1);
	if((rc = blocks.take(words*sizeof(unsigned long long), &tables))){ return rc; }
	a.bad = tables;
	a.out_off = tables + 1;
	a.bucket_n = (uint32_t*)(a.out_off + nq + 1);
	a.bucket_off = a.bucket_n + ((nq + 1) & ~1ull);
	if((rc = blocks.take(std::max<uint64_t>(n_hits, 1)*sizeof(unsigned long long), &a.keys))){ return rc; }
	if((rc = blocks.take(std::max<uint64_t>(n_hits, 1)*sizeof(uint32_t), &a.cols))){ return rc; }
	HIP_TRY(hipMemsetAsync(a.bad, 0, sizeof(unsigned long long), s));
	if(nq){ HIP_TRY(hipMemsetAsync(a.bucket_n, 0, nq*sizeof(uint32_t), s)); }
	const uint32_t stream_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(STREAM_BLOCKS_MAX, (n_hits + 255)/256));
	if(n_hits){
		hipLaunchKernelGGL(merge_count_kernel, dim3(stream_blocks), dim3(256), 0, s, a);
		HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(TM_SCAN_THREADS), 0, s, a);
	HIP_TRY(hipGetLastError());
	if(n_hits && nq){
		hipLaunchKernelGGL(merge_scatter_kernel, dim3(stream_blocks), dim3(256), 0, s, a);
		HIP_TRY(hipGetLastError());
		const size_t lds = (size_t)tm_pow2(k)*sizeof(unsigned long long);      // <= 8 KiB
		const uint32_t grid = std::min<uint32_t>(n_queries, SELECT_BLOCKS_MAX);
		if(select_block(n_hits, n_queries, k) == TM_WAVE){
			hipLaunchKernelGGL(merge_select_kernel<TM_WAVE>, dim3(grid), dim3(TM_WAVE), lds, s, a);
		}
		else{
			hipLaunchKernelGGL(merge_select_kernel<256>, dim3(grid), dim3(256), lds, s, a);
		}
		HIP_TRY(hipGetLastError());
	}
	unsigned long long bad = 0, total = 0;
	HIP_TRY(hipMemcpyAsync(&bad, a.bad, sizeof(bad), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(&total, a.out_count, sizeof(total), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if(bad){
		return fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: %llu records have a query >= n_queries (%u) or a column outside the order table (%llu entries)",
		            bad, n_queries, (unsigned long long)n_order);
	}
	if(total > out_capacity){
		return fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: the output has %llu records, out_capacity is %llu (the first %llu were written)",
		            total, (unsigned long long)out_capacity, (unsigned long long)out_capacity);
	}
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_topk_merge_device(kwage_ctx *ctx, const void *hits_dev, uint64_t n_hits, uint32_t n_queries, uint32_t k,
                                       const void *order_dev, uint64_t n_order, void *out_dev, uint64_t out_capacity,
                                       void *out_count_dev)
{
	if(!ctx || !out_count_dev || (n_hits && !hits_dev) || (out_capacity && !out_dev)){
		return kwage::fail(KWAGE_ERR_ARG, "kwage_topk_merge_device: NULL argument");
	}
	kwage::PoolBlocks blocks(&ctx->batch_pool);
	return kwage::settle(ctx, kwage::topk_merge(ctx, hits_dev, n_hits, n_queries, k, order_dev, n_order, out_dev, out_capacity,
	                                            out_count_dev, blocks));
}
