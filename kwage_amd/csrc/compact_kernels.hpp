// kwage_amd/csrc/compact_kernels.hpp -- the kernel of the compaction (compact.hip, kwage_group_compact): the surviving
// columns of every row of the RESIDENT matrix moved down into a dense prefix, IN PLACE.
#ifndef KWAGE_AMD_COMPACT_KERNELS_HPP
#define KWAGE_AMD_COMPACT_KERNELS_HPP

#include "compact_plan.hpp"

namespace kwage {

typedef uint32_t compact_v4 __attribute__((ext_vector_type(4)));      // 16 bytes as a clang vector: the nontemporal builtins take it

constexpr int COMPACT_THREADS = 256;

// compact_rows_kernel: in every row the units [first_unit, end_unit) are rewritten -- destination column d = source column
// of the run that covers d (compact_plan.hpp compact_unit), zero at and above column m.  `matrix` is read AND written: no
// __restrict__, no const alias for the loads.
//
// Ownership: a thread makes one 16-byte unit of one row per segment and stores it with one 16-byte store (the stride is
// a multiple of 128: every unit is whole and aligned) -- every byte is written once, by one thread: no atomics, nothing
// cleared beforehand.
//
// Why in place works: a destination column never lies above its source.  So every dword a unit loads lies at or above the
// unit's own first byte, and every load of segment j + 1 lies at or above the end of segment j: nothing the kernel reads
// was written earlier by the kernel.  What is left is write-after-read INSIDE a segment -- one thread's store may hit
// another thread's source -- and against it all threads of the workgroup make their unit of the segment in registers
// (the words are pinned there in front of the barrier: a value made from a load exists, so the load has returned), meet at
// __syncthreads() and only then store.  No second barrier before the next segment's loads, by the rule above; rows are
// independent, so the rows that share a workgroup are served by the same barrier.
//
// Every barrier is reached by every thread of the workgroup the same number of times: the loop over row groups strides
// by the grid (uniform per workgroup), the loop over segments runs `segments` times, and a thread without a unit (a row
// beyond the matrix, a unit beyond end_unit) makes nothing, arrives, and stores nothing.
__global__ __launch_bounds__(COMPACT_THREADS) void compact_rows_kernel(
	uint8_t *matrix, uint64_t stride, uint64_t nrows,
	const SaveRun *__restrict__ runs, uint32_t n_runs, uint32_t m,        // the plan; m surviving columns
	uint64_t first_unit, uint64_t end_unit,
	uint32_t lanes, uint32_t lanes_log2, uint64_t segments)                // compact_plan.hpp compact_schedule
{
	const uint64_t matrix_bytes = nrows*stride;
	const uint32_t rows_per_wg = COMPACT_THREADS >> lanes_log2;
	const uint32_t lane = threadIdx.x & (lanes - 1), sub = threadIdx.x >> lanes_log2;
	const uint64_t row_groups = (nrows + rows_per_wg - 1)/rows_per_wg;
	auto load = [&](uint64_t byte) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(matrix + byte)); };
	auto load4 = [&](uint64_t byte) {
		const compact_v4 q = __builtin_nontemporal_load(reinterpret_cast<const compact_v4*>(matrix + byte));
		return SaveQuad{q.x, q.y, q.z, q.w};
	};
	for(uint64_t rg = blockIdx.x; rg < row_groups; rg += gridDim.x){
		const uint64_t row = rg*rows_per_wg + sub;
		for(uint64_t seg = 0; seg < segments; ++seg){
			const uint64_t u = compact_unit_of(first_unit, seg, lanes, lane);
			const bool mine = row < nrows && u < end_unit;
			uint32_t w[4] = {0u, 0u, 0u, 0u};
			if(mine){ compact_unit(load, load4, runs, n_runs, m, row, stride, matrix_bytes, u, w); }
#pragma unroll
			for(int i = 0; i < 4; ++i){ asm volatile("" : "+v"(w[i])); }
			__syncthreads();
			if(mine){ *reinterpret_cast<uint4*>(matrix + row*stride + 16*u) = make_uint4(w[0], w[1], w[2], w[3]); }
		}
	}
}

}  // namespace kwage

#endif
