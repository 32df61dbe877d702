// kwage_amd/csrc/topk.hip -- kwage_search_topk (include/kwage_amd.h): for every query of a batch the k columns of a
// group with the highest k-mer counts, selected on the device.  No counterpart in the reference.
//
//   kmer_kernel  ->  topk_tile_kernel                                   ->  topk_merge_kernel  ->  D2H of <= k records per query
//               |->  count_kernel<SEG> + topk_combine_kernel (long queries)
//
// The batch layout, the k-mer stage, the counter widths, the segment rule and the result block are engine.hip's
// (declared in engine_state.hpp), as are the host-side objects (context, group, batch); the k-mer stage into blocks of
// the call is pool_blocks.hpp's, the launches and the slice driver are tile_search.hpp's (shared with scores.hip).  Of
// kernels.hpp this unit instantiates count_kernel's SEG form and the device functions topk_kernels.hpp builds on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "kwage_amd.h"
#include "engine_state.hpp"
#include "pool_blocks.hpp"
#include "kernels.hpp"
#include "topk_kernels.hpp"
#include "tile_search.hpp"

namespace kwage {
namespace {

struct TopkKernels {
	using Epi = TopkArgs;
	static constexpr const char *tile_name = "topk_tile_kernel<%u,%u>+topk_merge_kernel";
	static constexpr const char *seg_name = "count_kernel<%u,%u>+topk_combine_kernel<%u>+topk_merge_kernel";
	template <int PLANES, int NH> static auto tile() { return topk_tile_kernel<PLANES, NH>; }
	template <int PLANES> static auto combine() { return topk_combine_kernel<PLANES>; }      // (its grid is flat: any number of queries)
};

static const uint64_t CAND_BYTES_PER_SLICE = 256ull << 20;     // candidate keys of one slice of the batch's queries

// What the selection stage leaves on the device: per query (batch order) the k-mer count, the floor and the number of
// records selected, and up to k records per query in d_out[q*k ...], ordered by column (columns local to the group).
struct TopkSelection {
	uint32_t *d_nkmer = nullptr, *d_qthr = nullptr, *d_out_n = nullptr;
	unsigned long long *d_missing = nullptr;      // sparse groups: row indices not among the group's rows
	kwage_hit *d_out = nullptr;
	uint32_t launches = 0;                        // 0: nothing was selected (no queries or no columns); d_out_n is unset
	char kernel_name[64] = "";
};

// The selection stage of kwage_search_topk and kwage_search_topk_device_append: k-mer stage, tile kernels (or segments
// + combine) and the per-query merge, queued on the context's first stream and not waited for.
int topk_select(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, PoolBlocks &blocks, Events<4> &ev,
                TopkSelection &sel)
{
	kwage_ctx *ctx = g->ctx;
	int rc;
	if((rc = set_device(ctx))){ return rc; }
	const KmerLayout *L = nullptr;
	if((rc = batch_prepare(b, g->params.kmer_len, &L))){ return rc; }
	hipStream_t s = ctx->stream;
	const uint32_t n = b->n;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	const bool timing_kmer = timing && (flags & KWAGE_SEARCH_TIMING_KMER);
	// the launches' shapes: a slice of the queries holds CAND_BYTES_PER_SLICE of candidate keys at most
	const uint64_t cand_per_q = (uint64_t)tile_chunks(g)*k*sizeof(unsigned long long);
	const bool any = n && g->num_columns;
	TilePlan plan;
	if((rc = plan_tiles(g, L->max_pos, any ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, CAND_BYTES_PER_SLICE/cand_per_q)) : 0, 0, &plan))){ return rc; }
	if(timing && (rc = ev.create())){ return rc; }

	// ---- k-mer stage: distinct canonical k-mers, row indices, the floor (unsigned)(t * n) of every query --------------
	// (the floor at t = 1 is n: no complete_match here.  kwage_search reports 0 there, its AND path has no floor)
	KmerBlocks kb;
	if((rc = kmer_prologue(g, b, L, threshold, true, true, timing_kmer ? ev.ev : nullptr, blocks, s, &kb))){ return rc; }
	sel.d_nkmer = kb.nkmer;
	sel.d_qthr = kb.qthr;
	sel.d_out_n = kb.extra;
	sel.d_missing = kb.missing;
	if((rc = blocks.take(std::max<uint64_t>((uint64_t)n*k, 1)*sizeof(kwage_hit), &sel.d_out))){ return rc; }

	// ---- selection: tile kernels (or segments + combine) and the per-query merge, slice by slice of the queries --------
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[2], s)); }
	if(any){
		TopkArgs t;
		t.k = k;
		t.tiles = plan.chunks;
		if((rc = blocks.take((uint64_t)plan.slice*cand_per_q, &t.cand))){ return rc; }
		if((rc = blocks.take((uint64_t)plan.slice*plan.chunks*sizeof(uint32_t), &t.cand_n))){ return rc; }
		const RowListView v = {kb.rows, L->d_pos_off, kb.nkmer, n, L->max_pos, g->params.num_hash};
		rc = run_tile_slices<TopkKernels>(g, v, kb.qthr, plan, t, blocks, sel.kernel_name, s, [&](const SearchArgs &a, uint32_t q0) -> int {
			hipLaunchKernelGGL(topk_merge_kernel, dim3(a.n_queries), dim3(MERGE_THREADS), 0, s, t, q0, sel.d_out + (uint64_t)q0*k, sel.d_out_n + q0);
			HIP_TRY(hipGetLastError());
			++sel.launches;
			return KWAGE_OK;
		});
		if(rc){ return rc; }
	}
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[3], s)); }
	return KWAGE_OK;
}

int topk_check(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, const char *what)
{
	int rc;
	if((rc = search_check(g, b))){ return rc; }
	if(k < 1 || k > KWAGE_TOPK_MAX){ return fail(KWAGE_ERR_ARG, "%s: k must satisfy 1 <= k <= %u (got %u)", what, (unsigned)KWAGE_TOPK_MAX, k); }
	if(!(threshold >= 0.0f && threshold <= 1.0f)){ return fail(KWAGE_ERR_ARG, "%s: threshold must satisfy 0 <= t <= 1", what); }
	return KWAGE_OK;
}

int search_topk(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, PoolBlocks &blocks, kwage_result **out)
{
	int rc;
	if((rc = topk_check(g, b, k, threshold, "kwage_search_topk"))){ return rc; }
	Events<4> ev;
	TopkSelection sel;
	if((rc = topk_select(g, b, k, threshold, flags, blocks, ev, sel))){ return rc; }
	kwage_ctx *ctx = g->ctx;
	hipStream_t s = ctx->stream;
	const uint32_t n = b->n;
	const uint32_t nh = g->params.num_hash;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	const bool timing_kmer = timing && (flags & KWAGE_SEARCH_TIMING_KMER);
	uint32_t *d_nkmer = sel.d_nkmer, *d_qthr = sel.d_qthr, *d_out_n = sel.d_out_n;
	unsigned long long *d_missing = sel.d_missing;
	kwage_hit *d_out = sel.d_out;
	const uint32_t launches = sel.launches;

	// ---- copy back: per-query arrays, missing-row counter, the <= k records per query -----------------------------------
	std::unique_ptr<ResultStorage> rs(new (std::nothrow) ResultStorage());
	if(!rs){ return fail(KWAGE_ERR_DEVICE, "out of host memory"); }
	rs->nkmer.assign(n, 0);
	rs->qthr.assign(n, 0);
	std::vector<uint32_t> out_n(n, 0);
	std::vector<kwage_hit> staged((size_t)n*k);
	unsigned long long missing = 0;
	if(n){
		HIP_TRY(hipMemcpyAsync(rs->nkmer.data(), d_nkmer, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(rs->qthr.data(), d_qthr, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		if(launches){
			HIP_TRY(hipMemcpyAsync(out_n.data(), d_out_n, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipMemcpyAsync(staged.data(), d_out, (size_t)n*k*sizeof(kwage_hit), hipMemcpyDeviceToHost, s));
		}
		HIP_TRY(hipMemcpyAsync(&missing, d_missing, sizeof(missing), hipMemcpyDeviceToHost, s));
	}
	HIP_TRY(hipStreamSynchronize(s));
	if(missing){ return fail_missing_rows(missing); }
	uint64_t n_hits = 0, total_kmers = 0;
	for(uint32_t q = 0; q < n; ++q){ n_hits += std::min(out_n[q], k); total_kmers += rs->nkmer[q]; }
	rs->hits.reset(new (std::nothrow) kwage_hit[std::max<uint64_t>(n_hits, 1)]);
	if(!rs->hits){ return fail(KWAGE_ERR_DEVICE, "out of host memory (%llu hits)", (unsigned long long)n_hits); }
	uint64_t at = 0;
	for(uint32_t q = 0; q < n; ++q){
		const uint32_t m = std::min(out_n[q], k);
		memcpy(rs->hits.get() + at, staged.data() + (size_t)q*k, (size_t)m*sizeof(kwage_hit));
		at += m;
	}
	kwage_result &r = rs->pub;
	r.n_hits = n_hits;
	r.hits = rs->hits.get();
	r.n_queries = n;
	r.num_query_kmer = rs->nkmer.data();
	r.query_threshold = rs->qthr.data();
	r.total_kmers = total_kmers;
	r.bit_tests = total_kmers*nh*g->num_columns;
	r.algorithmic_bytes = total_kmers*nh*((g->num_columns + 7)/8);
	r.kmer_kernel_ms = 0;
	r.search_kernel_ms = 0;
	if(timing_kmer){ HIP_TRY(hipEventElapsedTime(&r.kmer_kernel_ms, ev.ev[0], ev.ev[1])); }
	if(timing){ HIP_TRY(hipEventElapsedTime(&r.search_kernel_ms, ev.ev[2], ev.ev[3])); }
	r.search_kernel_launches = launches;
	memcpy(rs->kernel, sel.kernel_name, sizeof(rs->kernel));
	r.search_kernel = rs->kernel;
	*out = &rs.release()->pub;
	return KWAGE_OK;
}

int search_topk_device_append(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, void *hits_dev,
                              uint64_t capacity, void *count_dev, uint32_t column_base, int reset_count,
                              void *num_query_kmer_dev, PoolBlocks &blocks, uint64_t *n_total)
{
	int rc;
	if((rc = topk_check(g, b, k, threshold, "kwage_search_topk_device_append"))){ return rc; }
	if((uint64_t)column_base + g->stride*8 > 0x100000000ull){
		return fail(KWAGE_ERR_ARG, "kwage_search_topk_device_append: column base %u + the group's column span exceeds 32 bits", column_base);
	}
	Events<4> ev;
	TopkSelection sel;
	if((rc = topk_select(g, b, k, threshold, flags & ~(uint32_t)(KWAGE_SEARCH_TIMING | KWAGE_SEARCH_TIMING_KMER), blocks, ev, sel))){ return rc; }
	hipStream_t s = g->ctx->stream;
	const uint32_t n = b->n;
	std::vector<uint32_t> out_n(n, 0);
	unsigned long long missing = 0, base = 0;
	if(sel.launches){ HIP_TRY(hipMemcpyAsync(out_n.data(), sel.d_out_n, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s)); }
	HIP_TRY(hipMemcpyAsync(&missing, sel.d_missing, sizeof(missing), hipMemcpyDeviceToHost, s));
	if(!reset_count){ HIP_TRY(hipMemcpyAsync(&base, count_dev, sizeof(base), hipMemcpyDeviceToHost, s)); }
	HIP_TRY(hipStreamSynchronize(s));
	if(missing){ return fail_missing_rows(missing); }
	// the output offsets of the queries, in batch order: the list grows by query, then column, behind what it held
	std::vector<unsigned long long> off(std::max<uint32_t>(n, 1), 0);
	unsigned long long added = 0;
	for(uint32_t q = 0; q < n; ++q){ off[q] = added; added += std::min(out_n[q], k); }
	const unsigned long long total = base + added;
	if(added){
		unsigned long long *d_off = nullptr;
		if((rc = blocks.take((uint64_t)n*sizeof(unsigned long long), &d_off))){ return rc; }
		HIP_TRY(hipMemcpyAsync(d_off, off.data(), (size_t)n*sizeof(unsigned long long), hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(topk_append_kernel, dim3(n), dim3(WAVE), 0, s, sel.d_out, sel.d_out_n, k, d_off, base,
		                   column_base, (kwage_hit*)hits_dev, (unsigned long long)capacity);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(count_dev, &total, sizeof(total), hipMemcpyHostToDevice, s));
	if(num_query_kmer_dev && n){
		HIP_TRY(hipMemcpyAsync(num_query_kmer_dev, sel.d_nkmer, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
	}
	HIP_TRY(hipStreamSynchronize(s));
	*n_total = total;
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_search_topk(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, kwage_result **out)
{
	if(!g || !b || !out){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_topk: NULL argument"); }
	*out = nullptr;
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_topk(g, b, k, threshold, flags, blocks, out));
}

extern "C" int kwage_search_topk_device_append(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags,
                                               void *hits_dev, uint64_t capacity, void *count_dev, uint32_t column_base,
                                               int reset_count, void *num_query_kmer_dev, uint64_t *n_total)
{
	if(!g || !b || !count_dev || !n_total || (capacity && !hits_dev)){
		return kwage::fail(KWAGE_ERR_ARG, "kwage_search_topk_device_append: NULL argument");
	}
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::search_topk_device_append(g, b, k, threshold, flags, hits_dev, capacity, count_dev, column_base,
	                                                              reset_count, num_query_kmer_dev, blocks, n_total));
}
