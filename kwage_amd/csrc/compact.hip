// kwage_amd/csrc/compact.hip -- compaction: the gaps that retired columns and alignment pads leave in a group's RESIDENT
// matrix closed in place -- every row's surviving columns move down into a dense prefix, the span shrinks, and the freed
// capacity is the next insert's at once.  What retire (insert.hip) does not do, without the round trip through a file that
// the save (save.hip) needs.  No counterpart in the reference.
//
//   what moves where           compact_plan.hpp plan_compact: the valid columns folded into runs (save_plan.hpp's), the units
//                              of a row that are rewritten, the schedule of a row
//   who writes what, and when  compact_kernels.hpp compact_rows_kernel: one thread per 16-byte unit, a segment's units all
//                              made before any is stored
//   the state a call leaves    h_valid / d_valid = bits [0, m), next_byte = ceil(m / 8), the tail open at m, and -- for a
//                              finalized group -- density / density_max re-sampled with finalize's probe (loader.hip)
//
// Every refusal is found before a byte is written.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "compact_kernels.hpp"
#include "compact_plan.hpp"
#include "engine_state.hpp"

using namespace kwage;

// loader.hip
namespace kwage { void group_probe_density(kwage_group *g); }

namespace {

// compact_rows_kernel over all rows, queued on `stream`: rows of COMPACT_THREADS units and more to rewrite take a workgroup
// each, segment after segment; narrower ones share one.
hipError_t launch_compact(kwage_group *g, const SaveRun *d_runs, const CompactPlan &plan, hipStream_t stream)
{
	const CompactSchedule s = compact_schedule(plan.first_unit, plan.end_unit, COMPACT_THREADS);
	uint32_t lanes_log2 = 0;
	while((1u << lanes_log2) < s.lanes){ ++lanes_log2; }
	const uint64_t row_groups = (g->nrows + s.rows_per_wg - 1)/s.rows_per_wg;
	const dim3 grid((uint32_t)std::min<uint64_t>(row_groups, (uint64_t)std::max(g->ctx->ncu, 1)*8)), block(COMPACT_THREADS);
	hipLaunchKernelGGL(compact_rows_kernel, grid, block, 0, stream, g->d_bits, g->stride, g->nrows, d_runs, (uint32_t)plan.runs.size(),
	                   (uint32_t)plan.m, plan.first_unit, plan.end_unit, s.lanes, lanes_log2, s.segments);
	return hipGetLastError();
}

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

}  // namespace

extern "C" int kwage_group_compact(kwage_group *g, uint32_t flags, uint64_t *new_column, uint64_t capacity, kwage_compact_stats *stats)
{
	const char *who = "kwage_group_compact";
	if(!g){ return fail(KWAGE_ERR_ARG, "%s: NULL group", who); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group is not compacted", who); }
	kwage_ctx *ctx = g->ctx;
	for(int i = 0; i < 2; ++i){ if(ctx->slot[i].busy){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); } }
	const uint64_t old_bytes = g->next_byte, span = old_bytes*8;
	CompactPlan plan;
	int rc = plan_compact(g->h_valid.data(), span, g->tail_open, g->tail_column, new_column != nullptr, capacity, plan);
	if(rc){ return rc; }
	if((rc = set_device(ctx))){ return rc; }
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	float kernel_ms = 0;
	if(plan.end_unit > plan.first_unit){
		Events ev;
		if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
		DevBuf d_runs;
		if((rc = d_runs.reserve(plan.runs.size()*sizeof(SaveRun)))){ return rc; }
		hipError_t e = hipMemcpyAsync(d_runs.p, plan.runs.data(), plan.runs.size()*sizeof(SaveRun), hipMemcpyHostToDevice, ctx->stream);
		if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev0, ctx->stream); }
		if(e == hipSuccess){ e = launch_compact(g, (const SaveRun*)d_runs.p, plan, ctx->stream); }
		if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev1, ctx->stream); }
		if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
		if(e == hipSuccess && timing){ (void)hipEventElapsedTime(&kernel_ms, ev.ev0, ev.ev1); }
		d_runs.release();
		if(e != hipSuccess){ return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
	}
	// the survivors are columns 0 .. m - 1: the group's state follows (the map is made from the mask as it was)
	if(new_column){ compact_fill_map(g->h_valid.data(), span, new_column); }
	compact_valid_mask(g->h_valid.data(), old_bytes, plan.m);
	g->next_byte = (plan.m + 7)/8;
	g->tail_column = plan.m;
	g->tail_open = true;
	if(old_bytes){ HIP_TRY(hipMemcpyAsync(g->d_valid, g->h_valid.data(), old_bytes, hipMemcpyHostToDevice, ctx->stream)); }
	if(g->finalized){ group_probe_density(g); }
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(stats){
		stats->span_before = span;
		stats->span_after = g->next_byte*8;
		stats->columns = plan.m;
		stats->runs = plan.runs.size();
		stats->first_unit = plan.first_unit;
		stats->units = plan.end_unit - plan.first_unit;
		stats->kernel_ms = kernel_ms;
	}
	return KWAGE_OK;
}
