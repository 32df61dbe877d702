// kwage_amd/csrc/union.hip -- the union of columns: new columns of a RESIDENT group, each the row-wise OR of listed
// columns of a resident group (the same one, or another with the same parameters), made on the device in one pass --
// the Bloom filter of the union of the members' k-mer sets, byte for byte the filter built from all their reads together,
// without the two transposes and the host image of an export, an OR on the host and an insert.  No counterpart in the
// reference.
//
//   what goes where            union_plan.hpp plan_union: the member lists folded into (source dword, mask) entries, the
//                              place in the destination (insert_plan.hpp plan_insert; within one group the next 16-byte
//                              boundary of the row also behind an open tail), the units of a row written
//   who writes what            union_kernels.hpp union_columns_kernel: one lane per (destination row, 16-byte unit)
//   the state a call leaves    the source's columns untouched; the destination as commit_insert (insert.hip) leaves it after
//                              an insert of the same filters at the same place
//
// Every refusal is found before a byte is written or allocated.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine_state.hpp"
#include "union_kernels.hpp"
#include "union_plan.hpp"

using namespace kwage;

// insert.hip
namespace kwage { int commit_insert(kwage_group *g, uint64_t first, uint64_t n); }

namespace {

// union_columns_kernel over all rows, queued on `stream` (the copy's launch cap).
hipError_t launch_union(const kwage_group *src, kwage_group *dst, const UnionEntry *d_entries, const uint32_t *d_offsets, const UnionPlan &plan, hipStream_t stream)
{
	const uint64_t total = dst->nrows*plan.units;
	const dim3 grid((uint32_t)std::min<uint64_t>((total + UNION_THREADS - 1)/UNION_THREADS, 1u << 20)), block(UNION_THREADS);
	hipLaunchKernelGGL(union_columns_kernel, grid, block, 0, stream, (const uint8_t*)src->d_bits, src->stride, dst->d_bits, dst->stride, dst->nrows,
	                   d_entries, d_offsets, plan.first, plan.n, plan.first_unit, plan.units);
	return hipGetLastError();
}

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

CopySide side_of(const kwage_group *g) { return CopySide{g->ctx, g->d_row_map != nullptr, g->params}; }

}  // namespace

extern "C" int kwage_group_union_columns(kwage_group *dst, kwage_group *src, const uint64_t *columns, const uint64_t *set_offsets, uint32_t n_sets,
                                         uint32_t flags, uint64_t *first_column, kwage_union_stats *stats)
{
	const char *who = "kwage_group_union_columns";
	CopySide d{}, s{};
	bool pending = false;
	if(dst && src){      // (neither is looked into while the other is NULL)
		d = side_of(dst);
		s = side_of(src);
		for(int i = 0; i < 2; ++i){ pending = pending || dst->ctx->slot[i].busy; }
	}
	int rc = union_refusal(dst ? &d : nullptr, src ? &s : nullptr, columns != nullptr, set_offsets, first_column != nullptr, n_sets, pending);
	if(rc){ return rc; }
	UnionPlan plan;
	if((rc = plan_union(columns, set_offsets, n_sets, src->next_byte*8, src->h_valid.data(), dst == src,
	                    dst->next_byte, dst->tail_open, dst->tail_column, dst->stride, plan))){ return rc; }
	kwage_ctx *ctx = dst->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	float kernel_ms = 0;
	// one table: the entries (16 bytes each), the offsets behind them
	const uint64_t entry_bytes = plan.entries.size()*sizeof(UnionEntry), offset_bytes = plan.offsets.size()*sizeof(uint32_t);
	DevBuf d_plan;
	if((rc = d_plan.reserve(entry_bytes + offset_bytes))){ return rc; }
	uint8_t *base = (uint8_t*)d_plan.p;
	hipError_t e = hipMemcpyAsync(base, plan.entries.data(), entry_bytes, hipMemcpyHostToDevice, ctx->stream);
	if(e == hipSuccess){ e = hipMemcpyAsync(base + entry_bytes, plan.offsets.data(), offset_bytes, hipMemcpyHostToDevice, ctx->stream); }
	if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev0, ctx->stream); }
	if(e == hipSuccess){ e = launch_union(src, dst, (const UnionEntry*)base, (const uint32_t*)(base + entry_bytes), plan, ctx->stream); }
	if(e == hipSuccess && timing){ e = hipEventRecord(ev.ev1, ctx->stream); }
	if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
	if(e == hipSuccess && timing){ (void)hipEventElapsedTime(&kernel_ms, ev.ev0, ev.ev1); }
	d_plan.release();
	if(e != hipSuccess){ return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
	// the columns are in the matrix as an insert's would be: the destination's state follows (within one group the columns
	// skipped up to the 16-byte boundary stay what they were: pad columns)
	if((rc = commit_insert(dst, plan.first, plan.n))){ return rc; }
	if(stats){
		stats->first_column = plan.first;
		stats->sets = plan.n;
		stats->members = plan.members;
		stats->entries = plan.entries.size();
		stats->first_unit = plan.first_unit;
		stats->units = plan.units;
		stats->bytes_written = dst->nrows*plan.units*16;
		stats->kernel_ms = kernel_ms;
	}
	*first_column = plan.first;
	return KWAGE_OK;
}
