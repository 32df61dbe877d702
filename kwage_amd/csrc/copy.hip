// kwage_amd/csrc/copy.hip -- the copy between groups: listed columns of one RESIDENT group become new columns of another,
// packed on the device in one pass -- how a group grows (copy everything into a wider one), how groups that share their
// parameters merge, and how a working subset is split off, without the two transposes and the host image of an export
// followed by an insert.  No counterpart in the reference.
//
//   what goes where            copy_plan.hpp plan_copy: the list folded into runs (save_plan.hpp's), the place in the
//                              destination (insert_plan.hpp plan_insert: the live insert's rule), the units of a row written
//   who writes what            copy_kernels.hpp copy_columns_kernel: one lane per (destination row, 16-byte unit)
//   the state a call leaves    the source untouched; the destination as commit_insert (insert.hip) leaves it after an insert
//                              of the same columns: valid mask, span, open tail, column count, densities re-sampled if finalized
//
// Every refusal is found before a byte is written or allocated.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "copy_kernels.hpp"
#include "copy_plan.hpp"
#include "engine_state.hpp"

using namespace kwage;

// insert.hip
namespace kwage { int commit_insert(kwage_group *g, uint64_t first, uint64_t n); }

namespace {

// copy_columns_kernel over all rows, queued on `stream`.
hipError_t launch_copy(const kwage_group *src, kwage_group *dst, const SaveRun *d_runs, const CopyPlan &plan, hipStream_t stream)
{
	const uint64_t total = dst->nrows*plan.units;
	const dim3 grid((uint32_t)std::min<uint64_t>((total + COPY_THREADS - 1)/COPY_THREADS, 1u << 20)), block(COPY_THREADS);
	hipLaunchKernelGGL(copy_columns_kernel, grid, block, 0, stream, (const uint8_t*)src->d_bits, src->stride, dst->d_bits, dst->stride, dst->nrows,
	                   d_runs, (uint32_t)plan.runs.size(), plan.first, plan.n, plan.first_unit, plan.units);
	return hipGetLastError();
}

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

CopySide side_of(const kwage_group *g) { return CopySide{g->ctx, g->d_row_map != nullptr, g->params}; }

}  // namespace

extern "C" int kwage_group_copy_columns(kwage_group *dst, kwage_group *src, const uint64_t *columns, uint64_t n,
                                        uint32_t flags, uint64_t *first_column, kwage_copy_stats *stats)
{
	const char *who = "kwage_group_copy_columns";
	CopySide d{}, s{};
	bool pending = false;
	if(dst && src){      // (neither is looked into while the other is NULL)
		d = side_of(dst);
		s = side_of(src);
		for(int i = 0; i < 2; ++i){ pending = pending || dst->ctx->slot[i].busy; }
	}
	int rc = copy_refusal(dst ? &d : nullptr, src ? &s : nullptr, dst == src, first_column != nullptr, columns != nullptr, n, pending);
	if(rc){ return rc; }
	CopyPlan plan;
	if((rc = plan_copy(columns, n, src->next_byte*8, src->h_valid.data(), dst->next_byte, dst->tail_open, dst->tail_column, dst->stride, plan))){ return rc; }
	kwage_ctx *ctx = dst->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	float kernel_ms = 0;
	DevBuf d_runs;
	if((rc = d_runs.reserve(plan.runs.size()*sizeof(SaveRun)))){ return rc; }
	hipError_t e = hipMemcpyAsync(d_runs.p, plan.runs.data(), plan.runs.size()*sizeof(SaveRun), hipMemcpyHostToDevice, ctx->stream);
	if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev0, ctx->stream); }
	if(e == hipSuccess){ e = launch_copy(src, dst, (const SaveRun*)d_runs.p, plan, ctx->stream); }
	if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev1, ctx->stream); }
	if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
	if(e == hipSuccess && timing){ (void)hipEventElapsedTime(&kernel_ms, ev.ev0, ev.ev1); }
	d_runs.release();
	if(e != hipSuccess){ return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
	// the columns are in the matrix as an insert's would be: the destination's state follows
	if((rc = commit_insert(dst, plan.first, plan.n))){ return rc; }
	if(stats){
		stats->first_column = plan.first;
		stats->columns = plan.n;
		stats->runs = plan.runs.size();
		stats->first_unit = plan.first_unit;
		stats->units = plan.units;
		stats->bytes_written = dst->nrows*plan.units*16;
		stats->kernel_ms = kernel_ms;
	}
	*first_column = plan.first;
	return KWAGE_OK;
}
