// kwage_amd/csrc/fold.hip -- the fold: a NEW group whose Bloom filters are half, a quarter, .. 2^-f as long as those of a
// resident group, made on the device in one streaming pass -- the one group operation that changes a database's size per
// sample.  The reference takes a row index as hash % filter_len with a power-of-two length (kwage.cpp:411-412, :445), so
// the filter of a k-mer set at length 2^L' is the OR of the 2^(L - L') consecutive pieces of its filter at 2^L -- what the
// reference's own make_bloom_filter does to shorten a filter (make_bloom.cpp:344-354).  In the bit-sliced matrix that is
// row arithmetic: dst row r' = OR over j of src row r' + j * 2^L'.
//
//   what is read and written    fold_plan.hpp plan_fold: the units of a row, the items, the grid, the loads per item and pass
//   who writes what             fold_kernels.hpp fold_rows_kernel: one lane per 16-byte unit of a destination row
//   the state a call leaves     the source untouched; the new group with the source's column layout number for number --
//                               span, valid mask, tail, column count -- open or finalized as the source is
//
// Every refusal is found before anything is allocated.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_state.hpp"
#include "fold_kernels.hpp"
#include "fold_plan.hpp"

using namespace kwage;

// loader.hip
namespace kwage { void group_probe_density(kwage_group *g); }

namespace {

// fold_rows_kernel<J> over all items, queued on `stream`.
template <int J>
void launch_fold_as(const kwage_group *src, kwage_group *dst, const FoldPlan &plan, hipStream_t stream)
{
	hipLaunchKernelGGL(fold_rows_kernel<J>, dim3(plan.grid), dim3(FOLD_THREADS), 0, stream, (const uint8_t*)src->d_bits, dst->d_bits, src->stride,
	                   plan.units_per_row, plan.items, plan.chunks, plan.src_step, plan.passes);
}
hipError_t launch_fold(const kwage_group *src, kwage_group *dst, const FoldPlan &plan, hipStream_t stream)
{
	switch(plan.J){
		case 1: launch_fold_as<1>(src, dst, plan, stream); break;
		case 2: launch_fold_as<2>(src, dst, plan, stream); break;
		default: launch_fold_as<3>(src, dst, plan, stream); break;
	}
	return hipGetLastError();
}

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

}  // namespace

extern "C" int kwage_group_fold(kwage_group *src, uint32_t log_2_filter_len, uint32_t flags, kwage_group **out, kwage_fold_stats *stats)
{
	const char *who = "kwage_group_fold";
	bool pending = false;
	if(src){ for(int i = 0; i < 2; ++i){ pending = pending || src->ctx->slot[i].busy; } }
	int rc = fold_refusal(src != nullptr, out != nullptr, src && src->d_row_map, src ? src->params.log_2_filter_len : 0, log_2_filter_len, pending);
	if(rc){ return rc; }
	kwage_ctx *ctx = src->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const FoldPlan plan = plan_fold(src->params.log_2_filter_len, log_2_filter_len, src->next_byte, src->stride, ctx->ncu);
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	// the new group: kwage_group_create's path (placement, zero-initialised), a capacity of 8 * stride columns: the same stride
	kwage_params params = src->params;
	params.log_2_filter_len = log_2_filter_len;
	kwage_group *g = nullptr;
	if((rc = kwage_group_create(ctx, &params, src->stride*8, &g))){ return rc; }
	float kernel_ms = 0;
	hipError_t e = hipSuccess;
	if(plan.grid){
		if(timing){ e = hipEventRecord(ev.ev0, ctx->stream); }
		if(e == hipSuccess){ e = launch_fold(src, g, plan, ctx->stream); }
		if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev1, ctx->stream); }
		if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
		if(e == hipSuccess && timing){ (void)hipEventElapsedTime(&kernel_ms, ev.ev0, ev.ev1); }
	}
	// the column layout is the source's, number for number
	if(e == hipSuccess){
		g->next_byte = src->next_byte;
		g->tail_column = src->tail_column;
		g->tail_open = src->tail_open;
		g->num_columns = src->num_columns;
		g->h_valid = src->h_valid;
		e = hipMemcpyAsync(g->d_valid, g->h_valid.data(), g->stride, hipMemcpyHostToDevice, ctx->stream);
	}
	if(e == hipSuccess && src->finalized){
		g->finalized = true;
		group_probe_density(g);
	}
	if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
	if(e != hipSuccess){
		kwage_group_destroy(g);
		return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
	}
	if(stats){
		stats->log_2_before = plan.log_2_before;
		stats->log_2_after = plan.log_2_after;
		stats->units_per_row = plan.units_per_row;
		stats->bytes_read = plan.bytes_read;
		stats->bytes_written = plan.bytes_written;
		stats->kernel_ms = kernel_ms;
	}
	*out = g;
	return KWAGE_OK;
}
