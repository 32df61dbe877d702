// kwage_amd/csrc/overlap.hip -- the overlap matrix: for every pair of listed columns of two RESIDENT groups (or of one
// group against itself) the number of rows in which both are set -- shared(i, j) = popcount(col_i AND col_j), the matrix
// product M_a^T M_b of the bit matrices, formed on the matrix cores.  It answers "which samples resemble which" for all
// pairs at once, at a cost that does not depend on how full the filters are and without a row list.  No counterpart in
// the reference.
//
//   what goes where            overlap_plan.hpp plan_overlap: the lists cut into blocks of 32 columns (straight or
//                              gathered), the workgroup tiles and their order, the parts of the row range
//   who computes what          overlap_kernels.hpp overlap_mfma_kernel: one workgroup per (tile of 128 x 128 cells, part);
//                              overlap_combine_kernel sums the parts where there are several
//   the state a call leaves    both groups untouched
//
// Every refusal is found before a kernel runs or a byte is allocated.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "engine_state.hpp"
#include "overlap_kernels.hpp"
#include "overlap_launch.hpp"
#include "overlap_plan.hpp"
#include "pool_blocks.hpp"

using namespace kwage;

namespace kwage {

// The kernels of one product queued on s (overlap_launch.hpp): the tiles of every part, then -- several parts -- their sum.
int overlap_launch(hipStream_t s, const OverlapArgs &args)
{
	hipLaunchKernelGGL(overlap_mfma_kernel, dim3((uint32_t)((uint64_t)args.n_tiles*args.splits)), dim3(OVERLAP_THREADS), 0, s, args);
	HIP_TRY(hipGetLastError());
	if(args.splits > 1){
		hipLaunchKernelGGL(overlap_combine_kernel, dim3((uint32_t)((uint64_t)args.n_tiles*(OVERLAP_TILE_CELLS/OVERLAP_THREADS))), dim3(OVERLAP_THREADS), 0, s, args);
		HIP_TRY(hipGetLastError());
	}
	return KWAGE_OK;
}

namespace {

thread_local char last_kernel[64] = "";

int run_overlaps(const char *who, kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                 void *cells, uint64_t row_elems, uint32_t flags, kwage_overlap_stats *stats, bool host_form)
{
	last_kernel[0] = 0;
	CopySide sa{}, sb{};
	OverlapCall call{cells != nullptr, cols_a != nullptr, cols_b != nullptr, n_a, n_b, 0, 0, row_elems, false};
	// (no group is looked into while a refusal that needs none is due)
	const bool look = a && cells && (cols_a != nullptr) == (n_a != 0) && (cols_b != nullptr) == (n_b != 0) && (b || !cols_b);
	if(look){
		sa = overlap_side_of(a);
		call.span_a = a->next_byte*8;
		for(int i = 0; i < 2; ++i){ call.search_pending = call.search_pending || a->ctx->slot[i].busy; }
	}
	if(look && b){ sb = overlap_side_of(b); call.span_b = b->next_byte*8; }
	int rc = overlap_refusal(who, a ? &sa : nullptr, b ? &sb : nullptr, call);
	if(rc){ return rc; }
	kwage_ctx *ctx = a->ctx;
	OverlapPlan plan;
	if((rc = plan_overlap(who, cols_a, n_a, call.span_a, a->h_valid.data(), b != nullptr, cols_b, n_b, call.span_b, b ? b->h_valid.data() : nullptr,
	                      a->nrows, (uint32_t)std::max(ctx->ncu, 1), ctx->tune.overlap_splits, plan))){ return rc; }
	const uint64_t n_tiles = plan.tiles.size();
	float kernel_ms = 0;
	if(n_tiles){
		if((rc = set_device(ctx))){ return rc; }
		PoolBlocks blocks(&ctx->batch_pool);
		// one table: a's blocks, b's blocks, the tiles
		const uint64_t bytes_a = plan.blocks_a.size()*sizeof(OverlapBlock), bytes_b = plan.blocks_b.size()*sizeof(OverlapBlock), bytes_t = n_tiles*sizeof(OverlapTile);
		const uint64_t partial_bytes = overlap_partial_bytes(plan);
		uint8_t *d_table = nullptr;
		uint32_t *d_partial = nullptr, *d_cells = (uint32_t*)cells;
		if((rc = take_or_say(blocks, who, "the plan's tables", bytes_a + bytes_b + bytes_t, &d_table))){ return rc; }
		if(partial_bytes && (rc = take_or_say(blocks, who, "the parts' partial sums", partial_bytes, &d_partial))){ return rc; }
		if(host_form && (rc = take_or_say(blocks, who, "the cells", plan.n_a*plan.n_b*sizeof(uint32_t), &d_cells))){ return rc; }
		OverlapArgs args{};
		args.a_bits = a->d_bits; args.a_stride = a->stride;
		args.b_bits = b ? b->d_bits : a->d_bits; args.b_stride = b ? b->stride : a->stride;
		args.rows = plan.rows; args.groups = plan.groups;
		args.blocks_a = (const OverlapBlock*)d_table;
		args.blocks_b = b ? (const OverlapBlock*)(d_table + bytes_a) : args.blocks_a;
		args.n_blocks_a = (uint32_t)plan.blocks_a.size();
		args.n_blocks_b = b ? (uint32_t)plan.blocks_b.size() : args.n_blocks_a;
		args.tiles = (const OverlapTile*)(d_table + bytes_a + bytes_b);
		args.n_tiles = (uint32_t)n_tiles; args.splits = plan.splits;
		args.n_a = plan.n_a; args.n_b = plan.n_b;
		args.symmetric = plan.symmetric;
		args.cells = d_cells;
		args.row_elems = host_form ? plan.n_b : row_elems;
		args.partial = d_partial;
		auto body = [&]() -> int {
			HIP_TRY(hipMemcpyAsync(d_table, plan.blocks_a.data(), bytes_a, hipMemcpyHostToDevice, ctx->stream));
			if(bytes_b){ HIP_TRY(hipMemcpyAsync(d_table + bytes_a, plan.blocks_b.data(), bytes_b, hipMemcpyHostToDevice, ctx->stream)); }
			HIP_TRY(hipMemcpyAsync(d_table + bytes_a + bytes_b, plan.tiles.data(), bytes_t, hipMemcpyHostToDevice, ctx->stream));
			return KWAGE_OK;
		};
		if((rc = body())){ return settle(ctx, rc); }
		rc = timed_section((flags & KWAGE_SEARCH_TIMING) != 0, ctx->stream, &kernel_ms, [&]() -> int {
			return overlap_launch(ctx->stream, args);
		});
		if(rc){ return settle(ctx, rc); }
		if(host_form){
			hipError_t e = hipMemcpy2DAsync(cells, row_elems*sizeof(uint32_t), d_cells, plan.n_b*sizeof(uint32_t), plan.n_b*sizeof(uint32_t), plan.n_a,
			                                hipMemcpyDeviceToHost, ctx->stream);
			if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
			if(e != hipSuccess){ return settle(ctx, fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e))); }
		}
		snprintf(last_kernel, sizeof(last_kernel), "%s", plan.splits > 1 ? "overlap_mfma_kernel+overlap_combine_kernel" : "overlap_mfma_kernel");
	}
	if(stats){
		stats->n_a = plan.n_a; stats->n_b = plan.n_b; stats->rows = plan.rows;
		stats->tiles = n_tiles; stats->splits = plan.splits;
		stats->straight_blocks = plan.straight_blocks; stats->gathered_blocks = plan.gathered_blocks;
		stats->symmetric = plan.symmetric;
		stats->kernel_ms = kernel_ms;
	}
	return KWAGE_OK;
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_group_column_overlaps_device(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                                  void *cells_dev, uint64_t row_elems, uint32_t flags, kwage_overlap_stats *stats)
{
	return run_overlaps("kwage_group_column_overlaps_device", a, cols_a, n_a, b, cols_b, n_b, cells_dev, row_elems, flags, stats, false);
}

extern "C" int kwage_group_column_overlaps(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                           uint32_t *cells, uint64_t row_elems, uint32_t flags, kwage_overlap_stats *stats)
{
	return run_overlaps("kwage_group_column_overlaps", a, cols_a, n_a, b, cols_b, n_b, cells, row_elems, flags, stats, true);
}

extern "C" const char *kwage_group_overlap_kernel(void) { return kwage::last_kernel; }
