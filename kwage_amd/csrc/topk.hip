// kwage_amd/csrc/topk.hip -- kwage_search_topk (include/kwage_amd.h): for every query of a batch the k columns of a
// group with the highest k-mer counts, selected on the device.  No counterpart in the reference.
//
//   kmer_kernel  ->  topk_tile_kernel                                   ->  topk_merge_kernel  ->  D2H of <= k records per query
//               |->  count_kernel<SEG> + topk_combine_kernel (long queries)
//
// The batch layout, the k-mer stage, the counter widths, the segment rule and the result block are engine.hip's
// (declared in engine_state.hpp), as are the host-side objects (context, group, batch); of kernels.hpp this unit
// instantiates count_kernel's SEG form and the device functions topk_kernels.hpp builds on.
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

namespace kwage {
namespace {

struct Events {
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	~Events() { for(hipEvent_t e : ev){ if(e){ (void)hipEventDestroy(e); } } }
};

template <int PLANES, int NH>
void launch_tile(const SearchArgs &a, const TopkArgs &t, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a.n_queries*a.chunks;
	hipLaunchKernelGGL((topk_tile_kernel<PLANES, NH>), dim3((uint32_t)((tiles + 3)/4)), dim3(SEARCH_THREADS), 0, s, a, t);
}

template <int PLANES, int NH>
void launch_seg_count(const SearchArgs &a, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a.n_queries*a.segs*a.chunks;
	hipLaunchKernelGGL((count_kernel<PLANES, NH, true>), dim3((uint32_t)((tiles + 3)/4)), dim3(SEARCH_THREADS), 0, s, a);
}

template <int PLANES>
int launch_combine(const SearchArgs &a, const TopkArgs &t, uint32_t seg_planes, hipStream_t s)
{
	const size_t lds = (size_t)(COMBINE_WAVES/2)*PLANES*WAVE*16;
	if(lds > 48*1024){
		HIP_TRY(hipFuncSetAttribute((const void*)topk_combine_kernel<PLANES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	}
	hipLaunchKernelGGL((topk_combine_kernel<PLANES>), dim3(a.n_queries*a.chunks), dim3(COMBINE_WAVES*WAVE), lds, s, a, t, seg_planes);
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
template <int P, int NH> struct TileLaunch { static void run(const SearchArgs &a, const TopkArgs &t, hipStream_t s) { launch_tile<P, NH>(a, t, s); } };
template <int P, int NH> struct SegLaunch { static void run(const SearchArgs &a, hipStream_t s) { launch_seg_count<P, NH>(a, s); } };

static const uint64_t CAND_BYTES_PER_SLICE = 256ull << 20;     // candidate keys of one slice of the batch's queries
static const uint64_t SLAB_BYTES_PER_SLICE = 1ull << 30;       // partial counters of one slice (segmented form)

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
int topk_select(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, PoolBlocks &blocks, Events &ev,
                TopkSelection &sel)
{
	kwage_ctx *ctx = g->ctx;
	int rc;
	if((rc = set_device(ctx))){ return rc; }
	const KmerLayout *L = nullptr;
	if((rc = batch_prepare(b, g->params.kmer_len, &L))){ return rc; }
	const uint32_t nh = g->params.num_hash;
	if(L->max_pos*nh > 0xFFFFFFFFull){
		return fail(KWAGE_ERR_ARG, "a query of %llu k-mer positions x %u hash functions exceeds 2^32 rows", (unsigned long long)L->max_pos, nh);
	}
	hipStream_t s = ctx->stream;
	const uint32_t n = b->n;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	const bool timing_kmer = timing && (flags & KWAGE_SEARCH_TIMING_KMER);
	if(timing){ for(hipEvent_t &e : ev.ev){ HIP_TRY(hipEventCreate(&e)); } }

	uint32_t *d_rows = nullptr, *d_nkmer = nullptr, *d_qthr = nullptr, *d_out_n = nullptr;
	unsigned long long *d_tables = nullptr, *d_missing = nullptr;
	kwage_hit *d_out = nullptr;
	if((rc = blocks.take(std::max<uint64_t>(L->total_pos*nh, 1)*sizeof(uint32_t), &d_rows))){ return rc; }
	if((rc = blocks.take(std::max<uint64_t>(n, 1)*sizeof(uint32_t)*3 + 16, &d_nkmer))){ return rc; }
	d_qthr = d_nkmer + std::max<uint32_t>(n, 1);
	d_out_n = d_qthr + std::max<uint32_t>(n, 1);
	d_missing = (unsigned long long*)(((uintptr_t)(d_out_n + std::max<uint32_t>(n, 1)) + 7) & ~(uintptr_t)7);
	if((rc = blocks.take(std::max<uint64_t>((uint64_t)n*k, 1)*sizeof(kwage_hit), &d_out))){ return rc; }
	HIP_TRY(hipMemsetAsync(d_missing, 0, sizeof(unsigned long long), s));

	// ---- k-mer stage: distinct canonical k-mers, row indices, the floor (unsigned)(t * n) of every query --------------
	if(timing_kmer){ HIP_TRY(hipEventRecord(ev.ev[0], s)); }
	if(n){
		if(L->table_slots){
			if((rc = blocks.take(L->table_slots*sizeof(uint64_t), &d_tables))){ return rc; }
			HIP_TRY(hipMemsetAsync(d_tables, 0xFF, L->table_slots*sizeof(uint64_t), s));
		}
		// (the floor at t = 1 is n: no complete_match here.  kwage_search reports 0 there, its AND path has no floor)
		const KmerStageOut o = {d_rows, nullptr, d_nkmer, d_qthr, d_tables};
		if((rc = launch_kmer_kernels(g->params, b, L, threshold, 0, o, s))){ return rc; }
		if(g->d_row_map && (rc = launch_remap_rows(g, n, L, d_rows, d_nkmer, d_missing, s))){ return rc; }
	}
	if(timing_kmer){ HIP_TRY(hipEventRecord(ev.ev[1], s)); }

	// ---- selection: tile kernels (or segments + combine) and the per-query merge, slice by slice of the queries --------
	char kernel_name[64] = "";
	uint32_t launches = 0;
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[2], s)); }
	if(n && g->num_columns){
		SearchArgs a;
		memset(&a, 0, sizeof(a));
		a.db = g->d_bits;
		a.stride = g->stride;
		a.units_per_row = (uint32_t)(g->stride/16);
		a.valid = g->d_valid;
		a.rows = d_rows;
		a.num_hash = nh;
		a.chunks = (a.units_per_row + WAVE - 1)/WAVE;
		const uint32_t planes = planes_for(L->max_pos);
		const uint64_t cand_per_q = (uint64_t)a.chunks*k*sizeof(unsigned long long);
		uint32_t slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, CAND_BYTES_PER_SLICE/cand_per_q));
		a.n_queries = slice;
		choose_segments(a, L->max_pos, 1024, ctx->tune.force_segs);      // (topk_combine_kernel's grid is flat: any number of queries)
		uint32_t seg_planes = (a.segs > 1) ? planes_for(a.seg_kmers) : planes;
		if(a.segs > 1){      // keep the slab of partial counters bounded: fewer queries per slice
			const uint64_t slab_per_q = (uint64_t)a.segs*seg_planes*g->stride;
			slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slice, SLAB_BYTES_PER_SLICE/slab_per_q));
		}
		if((uint64_t)slice*a.segs*a.chunks/4 + 1 > 0x7FFFFFFFull){ return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
		TopkArgs t;
		t.k = k;
		t.tiles = a.chunks;
		if((rc = blocks.take((uint64_t)slice*cand_per_q, &t.cand))){ return rc; }
		if((rc = blocks.take((uint64_t)slice*a.chunks*sizeof(uint32_t), &t.cand_n))){ return rc; }
		if(a.segs > 1){
			uint32_t *slab = nullptr;
			if((rc = blocks.take((uint64_t)slice*a.segs*seg_planes*g->stride, &slab))){ return rc; }
			a.partial = slab;
			snprintf(kernel_name, sizeof(kernel_name), "count_kernel<%u,%u>+topk_combine_kernel<%u>+topk_merge_kernel", seg_planes, std::min(nh, 5u), planes);
		}
		else{
			snprintf(kernel_name, sizeof(kernel_name), "topk_tile_kernel<%u,%u>+topk_merge_kernel", planes, std::min(nh, 5u));
		}
		for(uint32_t q0 = 0; q0 < n; q0 += slice){
			a.n_queries = std::min(slice, n - q0);
			a.pos_off = L->d_pos_off + q0;
			a.nkmer = d_nkmer + q0;
			a.qthr = d_qthr + q0;
			if(a.segs > 1){
				by_shape<SegLaunch>(seg_planes, nh, a, s);
				HIP_TRY(hipGetLastError());
				switch(planes){
					case 7: rc = launch_combine<7>(a, t, seg_planes, s); break;
					case 10: rc = launch_combine<10>(a, t, seg_planes, s); break;
					case 14: rc = launch_combine<14>(a, t, seg_planes, s); break;
					case 20: rc = launch_combine<20>(a, t, seg_planes, s); break;
					default: rc = launch_combine<32>(a, t, seg_planes, s); break;
				}
				if(rc){ return rc; }
			}
			else{
				by_shape<TileLaunch>(planes, nh, a, t, s);
			}
			HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(topk_merge_kernel, dim3(a.n_queries), dim3(MERGE_THREADS), 0, s, t, q0, d_out + (uint64_t)q0*k, d_out_n + q0);
			HIP_TRY(hipGetLastError());
			++launches;
		}
	}
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[3], s)); }
	sel.d_nkmer = d_nkmer;
	sel.d_qthr = d_qthr;
	sel.d_out_n = d_out_n;
	sel.d_missing = d_missing;
	sel.d_out = d_out;
	sel.launches = launches;
	memcpy(sel.kernel_name, kernel_name, sizeof(sel.kernel_name));
	return KWAGE_OK;
}

int topk_check(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, const char *what)
{
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "kwage_group_finalize() must be called before searching"); }
	if(b->ctx != g->ctx){ return fail(KWAGE_ERR_ARG, "batch and group belong to different contexts"); }
	if(k < 1 || k > KWAGE_TOPK_MAX){ return fail(KWAGE_ERR_ARG, "%s: k must satisfy 1 <= k <= %u (got %u)", what, (unsigned)KWAGE_TOPK_MAX, k); }
	if(!(threshold >= 0.0f && threshold <= 1.0f)){ return fail(KWAGE_ERR_ARG, "%s: threshold must satisfy 0 <= t <= 1", what); }
	return KWAGE_OK;
}

int search_topk(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags, PoolBlocks &blocks, kwage_result **out)
{
	int rc;
	if((rc = topk_check(g, b, k, threshold, "kwage_search_topk"))){ return rc; }
	Events ev;
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
	if(missing){
		return fail(KWAGE_ERR_STATE, "%llu row indices of this batch are not among the rows of the sparse group (it was created for other queries)", missing);
	}
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
	Events ev;
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
	if(missing){
		return fail(KWAGE_ERR_STATE, "%llu row indices of this batch are not among the rows of the sparse group (it was created for other queries)", missing);
	}
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
	const int rc = kwage::search_topk(g, b, k, threshold, flags, blocks, out);
	if(rc){
		// an error return may leave kernels of this call queued: nothing of it may still run when `blocks` hands its
		// device memory back to the pool (its destructor, below)
		(void)hipStreamSynchronize(g->ctx->stream);
		(void)hipGetLastError();
	}
	return rc;
}

extern "C" int kwage_search_topk_device_append(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags,
                                               void *hits_dev, uint64_t capacity, void *count_dev, uint32_t column_base,
                                               int reset_count, void *num_query_kmer_dev, uint64_t *n_total)
{
	if(!g || !b || !count_dev || !n_total || (capacity && !hits_dev)){
		return kwage::fail(KWAGE_ERR_ARG, "kwage_search_topk_device_append: NULL argument");
	}
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	const int rc = kwage::search_topk_device_append(g, b, k, threshold, flags, hits_dev, capacity, count_dev, column_base,
	                                                reset_count, num_query_kmer_dev, blocks, n_total);
	if(rc){      // as kwage_search_topk: nothing of this call may still run when `blocks` hands its memory back
		(void)hipStreamSynchronize(g->ctx->stream);
		(void)hipGetLastError();
	}
	return rc;
}
