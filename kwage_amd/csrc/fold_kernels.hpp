// kwage_amd/csrc/fold_kernels.hpp -- the kernel of the fold (fold.hip, kwage_group_fold): every row of the SHORT matrix made
// as the OR of the 2^f rows of the resident long matrix that fall on it (row r' + j * 2^L'), one streaming pass.
#ifndef KWAGE_AMD_FOLD_KERNELS_HPP
#define KWAGE_AMD_FOLD_KERNELS_HPP

#include "fold_plan.hpp"

namespace kwage {

typedef uint32_t fold_v4 __attribute__((ext_vector_type(4)));      // 16 bytes as a clang vector: the nontemporal builtins take it

// fold_rows_kernel<J>: one lane per item (fold_plan.hpp: a 16-byte unit of a destination row).  A lane loads the item's
// sources, ORs them in registers and issues ONE 16-byte store: every destination byte is written once, by one lane, and
// the destination is never read -- no atomics, no LDS, nothing cleared (the bytes from 16 * units_per_row to the stride
// are the zeros the matrix was allocated with).  `src` and `dst` are different allocations.
//
// Eight 16-byte loads are requested per lane before any is waited for, whatever f is: 8 >> J items of 2^J loads each
// (f = 1: 4 items x 2 loads, f = 2: 2 x 4, f >= 3: 1 x 8), and for f > 3 2^(f - 3) such passes into the same
// accumulator.  Consecutive lanes hold consecutive items, so each of the eight requests of a wave covers up to 1 KiB of
// one source row.
//
// Workgroups of 256 lanes, at most 8 per compute unit, persistent and grid-stride over the chunks.  The kernel uses no LDS,
// so registers alone bound its occupancy: the compiler's report gives 86 to 122 VGPRs (the 32 of the data, the items'
// 64-bit addresses, the division), 4 to 5 waves per SIMD -- with 8 x 16 bytes outstanding per lane 128 KiB and more in
// flight per compute unit, above the ~50 KiB that 6.3 TB/s over 256 compute units at a latency of 2 us asks for.  No
// register bound is set: nothing measured says that more waves would pay.
//
// A chunk that is not whole -- the last one, or the only one of a matrix with fewer items than a workgroup takes --
// goes item by item through fold_item_value, each lane checking its own item numbers: no load is issued for an item at or
// beyond `items`.  The branch is uniform in the workgroup.
//
// L' == 0 with a large f is one destination row: units_per_row items, each a loop over 2^f rows.  Few lanes, long loops --
// that case only needs to be correct (it is a single row of a database nobody searches), and it takes this same kernel.
template <int J>
__global__ __launch_bounds__(FOLD_THREADS) void fold_rows_kernel(
	const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t stride,
	uint64_t units_per_row, uint64_t items, uint64_t chunks, uint64_t src_step, uint32_t passes)      // fold_plan.hpp plan_fold
{
	constexpr int LOADS = 1 << J, ITEMS = (int)FOLD_LOADS_IN_FLIGHT >> J;
	auto load4 = [&](uint64_t byte) { return __builtin_nontemporal_load(reinterpret_cast<const fold_v4*>(src + byte)); };
	for(uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x){
		if(fold_chunk_item(chunk, ITEMS, ITEMS - 1, FOLD_THREADS - 1) < items){
			uint64_t byte[ITEMS];
			fold_v4 acc[ITEMS];
#pragma unroll
			for(int i = 0; i < ITEMS; ++i){
				byte[i] = fold_item(fold_chunk_item(chunk, ITEMS, i, threadIdx.x), units_per_row, stride).byte;
				acc[i] = fold_v4{0u, 0u, 0u, 0u};
			}
			uint64_t at = 0;
			for(uint32_t p = 0; p < passes; ++p){
				fold_v4 v[ITEMS][LOADS];
#pragma unroll
				for(int i = 0; i < ITEMS; ++i){
#pragma unroll
					for(int j = 0; j < LOADS; ++j){ v[i][j] = load4(byte[i] + at + (uint64_t)j*src_step); }
				}
#pragma unroll
				for(int i = 0; i < ITEMS; ++i){
#pragma unroll
					for(int j = 0; j < LOADS; ++j){ acc[i] |= v[i][j]; }
				}
				at += (uint64_t)LOADS*src_step;
			}
#pragma unroll
			for(int i = 0; i < ITEMS; ++i){ *reinterpret_cast<fold_v4*>(dst + byte[i]) = acc[i]; }
		}
		else{
			for(int i = 0; i < ITEMS; ++i){
				const uint64_t item = fold_chunk_item(chunk, ITEMS, i, threadIdx.x);
				if(item >= items){ continue; }
				const uint64_t byte = fold_item(item, units_per_row, stride).byte;
				const FoldQuad q = fold_item_value([&](uint64_t b) { const fold_v4 x = load4(b); return FoldQuad{x.x, x.y, x.z, x.w}; },
				                                   byte, src_step, (uint64_t)passes*LOADS);
				*reinterpret_cast<fold_v4*>(dst + byte) = fold_v4{q.x, q.y, q.z, q.w};
			}
		}
	}
}

}  // namespace kwage

#endif
