// kwage_amd/csrc/neighbors.hip -- nearest-neighbour lists: for every listed column of a RESIDENT group its k best partners
// among the listed columns of another (or the same) group, by shared set bits or by Jaccard index, chosen on the device
// from the overlap matrix's cells.  The cells never leave the device and never exist all at once: a's list is cut into
// strips, a strip's cells are formed by the overlap kernels in one block of the context's pool and reduced to k records
// per row before the next strip overwrites them.  No counterpart in the reference.
//
//   what goes where            neighbors_plan.hpp plan_neighbors: the strips, per strip the overlap's tiles and parts
//   who computes what          overlap_kernels.hpp (through overlap_launch.hpp) the cells; neighbors_kernels.hpp the set
//                              bits of the columns, and neighbors_select_kernel: one workgroup per entry of the strip
//   the state a call leaves    both groups untouched
//
// Every refusal is found before a kernel runs or a byte is allocated.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "engine_state.hpp"
#include "neighbors_kernels.hpp"
#include "neighbors_plan.hpp"
#include "overlap_launch.hpp"
#include "pool_blocks.hpp"

using namespace kwage;

namespace kwage {
namespace {

thread_local char last_kernel[96] = "";

// The set bits of every column of g's span into bits (span rounded up to 32 counts), through `partial`.
struct BitsBlocks { uint32_t *bits = nullptr, *partial = nullptr; uint32_t dwords = 0, parts = 0; };

void bits_shape(const kwage_group *g, uint64_t span, BitsBlocks *b)
{
	b->dwords = (uint32_t)((span + 31)/32);
	const uint32_t slabs = (b->dwords + NEIGHBORS_BITS_THREADS - 1)/NEIGHBORS_BITS_THREADS;
	const uint64_t want = slabs ? (2048 + slabs - 1)/slabs : 1;
	b->parts = (uint32_t)std::max<uint64_t>(std::min<uint64_t>({want, std::max<uint64_t>(g->nrows/256, 1), NEIGHBORS_BITS_MAX_PARTS}), 1);
}

int bits_launch(const kwage_group *g, const BitsBlocks &b, hipStream_t s)
{
	if(!b.dwords){ return KWAGE_OK; }
	const uint32_t slabs = (b.dwords + NEIGHBORS_BITS_THREADS - 1)/NEIGHBORS_BITS_THREADS;
	hipLaunchKernelGGL(neighbors_bits_kernel, dim3(slabs*b.parts), dim3(NEIGHBORS_BITS_THREADS), 0, s, (const uint8_t*)g->d_bits, (unsigned long long)g->stride,
	                   (unsigned long long)g->nrows, b.dwords, b.parts, b.partial);
	HIP_TRY(hipGetLastError());
	const uint32_t columns = b.dwords*32;
	hipLaunchKernelGGL(neighbors_bits_sum_kernel, dim3((columns + NEIGHBORS_THREADS - 1)/NEIGHBORS_THREADS), dim3(NEIGHBORS_THREADS), 0, s, (const uint32_t*)b.partial, b.parts, columns, b.bits);
	HIP_TRY(hipGetLastError());
	return KWAGE_OK;
}

int run_neighbors(const char *who, kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                  uint32_t k, uint32_t metric, uint32_t min_shared, void *out, void *counts, uint32_t flags, kwage_neighbors_stats *stats, bool host_form)
{
	last_kernel[0] = 0;
	int rc;
	if((rc = neighbors_refusal(who, a != nullptr, out != nullptr, counts != nullptr, k, metric))){ return rc; }
	CopySide sa{}, sb{};
	OverlapCall call{true, cols_a != nullptr, cols_b != nullptr, n_a, n_b, 0, 0, ~0ull, false};      // (no row_elems to refuse)
	// (no group is looked into while a refusal that needs none is due)
	const bool look = (cols_a != nullptr) == (n_a != 0) && (cols_b != nullptr) == (n_b != 0) && (b || !cols_b);
	if(look){
		sa = overlap_side_of(a);
		call.span_a = a->next_byte*8;
		for(int i = 0; i < 2; ++i){ call.search_pending = call.search_pending || a->ctx->slot[i].busy; }
	}
	if(look && b){ sb = overlap_side_of(b); call.span_b = b->next_byte*8; }
	if((rc = overlap_refusal(who, &sa, b ? &sb : nullptr, call))){ return rc; }
	kwage_ctx *ctx = a->ctx;
	NeighborsPlan plan;
	if((rc = plan_neighbors(who, cols_a, n_a, call.span_a, a->h_valid.data(), b != nullptr, cols_b, n_b, call.span_b, b ? b->h_valid.data() : nullptr,
	                        a->nrows, (uint32_t)std::max(ctx->ncu, 1), ctx->tune.overlap_splits, ctx->tune.neighbors_strip_bytes, plan))){ return rc; }
	float kernel_ms = 0;
	uint64_t records = 0;
	if(plan.n_a){
		if((rc = set_device(ctx))){ return rc; }
		PoolBlocks blocks(&ctx->batch_pool);
		const bool other_group = b && b != a;
		const bool with_cells = plan.n_b != 0;
		// one table: a's blocks, b's blocks, the tiles of a full strip, those of a shorter last one, the columns of either list
		const uint64_t bytes_a = plan.blocks_a.size()*sizeof(OverlapBlock), bytes_b = plan.blocks_b.size()*sizeof(OverlapBlock);
		const uint64_t bytes_tf = plan.full.tiles.size()*sizeof(OverlapTile), bytes_tl = plan.last.tiles.size()*sizeof(OverlapTile);
		const uint64_t bytes_ca = plan.col_a.size()*sizeof(uint32_t), bytes_cb = plan.col_b.size()*sizeof(uint32_t);
		const uint64_t at_b = bytes_a, at_tf = at_b + bytes_b, at_tl = at_tf + bytes_tf, at_ca = at_tl + bytes_tl, at_cb = at_ca + bytes_ca;
		const uint64_t cells_bytes = plan.strip_entries*plan.pitch*sizeof(uint32_t);
		BitsBlocks ba, bb;
		bits_shape(a, call.span_a, &ba);
		if(other_group){ bits_shape(b, call.span_b, &bb); }
		uint8_t *d_table = nullptr;
		uint32_t *d_partial = nullptr, *d_cells = nullptr, *d_counts = (uint32_t*)counts;
		kwage_neighbor *d_out = (kwage_neighbor*)out;
		if((rc = take_or_say(blocks, who, "the plan's tables", at_cb + bytes_cb, &d_table))){ return rc; }
		if(plan.partial_bytes && with_cells && (rc = take_or_say(blocks, who, "the parts' partial sums", plan.partial_bytes, &d_partial))){ return rc; }
		if(with_cells && (rc = take_or_say(blocks, who, "a strip's cells", cells_bytes, &d_cells))){ return rc; }
		for(BitsBlocks *x : {&ba, &bb}){
			if(!x->dwords){ continue; }
			if((rc = take_or_say(blocks, who, "the columns' set bits", (uint64_t)x->dwords*32*sizeof(uint32_t), &x->bits))){ return rc; }
			if((rc = take_or_say(blocks, who, "the partial set bits", (uint64_t)x->parts*x->dwords*32*sizeof(uint32_t), &x->partial))){ return rc; }
		}
		if(host_form){
			if((rc = take_or_say(blocks, who, "the records", plan.n_a*k*sizeof(kwage_neighbor), &d_out))){ return rc; }
			if((rc = take_or_say(blocks, who, "the counts", plan.n_a*sizeof(uint32_t), &d_counts))){ return rc; }
		}
		std::vector<uint32_t> h_counts(plan.n_a);

		OverlapArgs args{};
		args.a_bits = a->d_bits; args.a_stride = a->stride;
		args.b_bits = b ? b->d_bits : a->d_bits; args.b_stride = b ? b->stride : a->stride;
		args.rows = plan.rows; args.groups = plan.groups;
		args.blocks_b = (const OverlapBlock*)(d_table + (b ? at_b : 0));
		args.n_blocks_b = (uint32_t)(b ? plan.blocks_b.size() : plan.blocks_a.size());
		args.n_b = plan.n_b;
		args.symmetric = 0;
		args.cells = d_cells;
		args.row_elems = plan.pitch;
		args.partial = d_partial;
		NeighborsArgs sel{};
		sel.cells = d_cells; sel.pitch = plan.pitch; sel.n_b = plan.n_b;
		sel.col_a = (const uint32_t*)(d_table + at_ca);
		sel.col_b = b ? (const uint32_t*)(d_table + at_cb) : sel.col_a;
		sel.bits_a = ba.bits;
		sel.bits_b = other_group ? bb.bits : ba.bits;
		sel.k = k; sel.metric = metric; sel.min_shared = min_shared;
		sel.skip_same = (flags & KWAGE_NEIGHBORS_SKIP_SELF) && !other_group ? 1u : 0u;
		sel.tie_bytes = plan.tie_bytes;
		sel.out = d_out; sel.counts = d_counts;

		bool combined = false;
		auto upload = [&]() -> int {
			HIP_TRY(hipMemcpyAsync(d_table, plan.blocks_a.data(), bytes_a, hipMemcpyHostToDevice, ctx->stream));
			if(bytes_b){ HIP_TRY(hipMemcpyAsync(d_table + at_b, plan.blocks_b.data(), bytes_b, hipMemcpyHostToDevice, ctx->stream)); }
			if(bytes_tf){ HIP_TRY(hipMemcpyAsync(d_table + at_tf, plan.full.tiles.data(), bytes_tf, hipMemcpyHostToDevice, ctx->stream)); }
			if(bytes_tl){ HIP_TRY(hipMemcpyAsync(d_table + at_tl, plan.last.tiles.data(), bytes_tl, hipMemcpyHostToDevice, ctx->stream)); }
			HIP_TRY(hipMemcpyAsync(d_table + at_ca, plan.col_a.data(), bytes_ca, hipMemcpyHostToDevice, ctx->stream));
			if(bytes_cb){ HIP_TRY(hipMemcpyAsync(d_table + at_cb, plan.col_b.data(), bytes_cb, hipMemcpyHostToDevice, ctx->stream)); }
			int r = bits_launch(a, ba, ctx->stream);
			if(!r && other_group){ r = bits_launch(b, bb, ctx->stream); }
			return r;
		};
		if((rc = upload())){ return settle(ctx, rc); }
		rc = timed_section((flags & KWAGE_SEARCH_TIMING) != 0, ctx->stream, &kernel_ms, [&]() -> int {
			for(uint64_t s = 0; s < plan.strips; ++s){
				const NeighborsShape &shape = neighbors_strip_shape(plan, s);
				const uint64_t first = neighbors_strip_first(plan, s);
				if(with_cells){
					// the strip's blocks of a's list: a strip starts at a multiple of 128 entries, four blocks
					args.blocks_a = (const OverlapBlock*)d_table + first/OVERLAP_BLOCK;
					args.n_blocks_a = (uint32_t)((shape.entries + OVERLAP_BLOCK - 1)/OVERLAP_BLOCK);
					args.n_a = shape.entries;
					args.tiles = (const OverlapTile*)(d_table + (&shape == &plan.last ? at_tl : at_tf));
					args.n_tiles = (uint32_t)shape.tiles.size();
					args.splits = shape.splits;
					int r = overlap_launch(ctx->stream, args);
					if(r){ return r; }
					combined = combined || shape.splits > 1;
				}
				sel.entries = shape.entries; sel.first_entry = first;
				hipLaunchKernelGGL(neighbors_select_kernel, dim3((uint32_t)std::min<uint64_t>(shape.entries, 1u << 20)), dim3(NEIGHBORS_THREADS), 0, ctx->stream, sel);
				HIP_TRY(hipGetLastError());
			}
			return KWAGE_OK;
		});
		if(rc){ return settle(ctx, rc); }
		hipError_t e = hipMemcpyAsync(h_counts.data(), d_counts, plan.n_a*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
		if(e == hipSuccess && host_form){ e = hipMemcpyAsync(out, d_out, plan.n_a*k*sizeof(kwage_neighbor), hipMemcpyDeviceToHost, ctx->stream); }
		if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
		if(e != hipSuccess){ return settle(ctx, fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e))); }
		if(host_form){ std::copy(h_counts.begin(), h_counts.end(), (uint32_t*)counts); }
		for(uint32_t c : h_counts){ records += c; }
		snprintf(last_kernel, sizeof(last_kernel), "%s%s", !with_cells ? "" : combined ? "overlap_mfma_kernel+overlap_combine_kernel+" : "overlap_mfma_kernel+", "neighbors_select_kernel");
	}
	if(stats){
		stats->n_a = plan.n_a; stats->n_b = plan.n_b; stats->rows = plan.rows;
		stats->strips = plan.strips; stats->strip_entries = plan.strip_entries;
		stats->tiles = plan.tiles; stats->records = records;
		stats->metric = metric;
		stats->kernel_ms = kernel_ms;
	}
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_group_column_neighbors_device(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                                   uint32_t k, uint32_t metric, uint32_t min_shared, void *out_dev, void *counts_dev, uint32_t flags,
                                                   kwage_neighbors_stats *stats)
{
	return run_neighbors("kwage_group_column_neighbors_device", a, cols_a, n_a, b, cols_b, n_b, k, metric, min_shared, out_dev, counts_dev, flags, stats, false);
}

extern "C" int kwage_group_column_neighbors(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                            uint32_t k, uint32_t metric, uint32_t min_shared, kwage_neighbor *out, uint32_t *counts, uint32_t flags,
                                            kwage_neighbors_stats *stats)
{
	return run_neighbors("kwage_group_column_neighbors", a, cols_a, n_a, b, cols_b, n_b, k, metric, min_shared, out, counts, flags, stats, true);
}

extern "C" const char *kwage_group_neighbors_kernel(void) { return kwage::last_kernel; }
