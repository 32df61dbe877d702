// kwage_amd/csrc/overlap_launch.hpp -- what overlap.hip and neighbors.hip share on the device side of a call: the launch
// of the overlap kernels (defined in overlap.hip, the one translation unit that holds them), a group as the refusals see
// it, and the block of a call that cannot be had.
#ifndef KWAGE_AMD_OVERLAP_LAUNCH_HPP
#define KWAGE_AMD_OVERLAP_LAUNCH_HPP

#include <hip/hip_runtime.h>

#include "engine_state.hpp"
#include "overlap_plan.hpp"
#include "pool_blocks.hpp"

namespace kwage {

// overlap_mfma_kernel over args.n_tiles x args.splits workgroups and, with several parts, overlap_combine_kernel, queued
// on s and not waited for.
int overlap_launch(hipStream_t s, const OverlapArgs &args);

inline CopySide overlap_side_of(const kwage_group *g) { return CopySide{g->ctx, g->d_row_map != nullptr, g->params}; }

// The block of a call that cannot be had: the pool's error with the size that was asked for.
template <typename T>
int take_or_say(PoolBlocks &blocks, const char *who, const char *what, uint64_t bytes, T **out)
{
	const int rc = blocks.take(bytes, out);
	if(rc){ return fail(rc, "%s: no device memory for the %llu bytes of %s", who, (unsigned long long)bytes, what); }
	return KWAGE_OK;
}

}  // namespace kwage

#endif
