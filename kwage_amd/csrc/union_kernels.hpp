// kwage_amd/csrc/union_kernels.hpp -- the kernel of the union of columns (union.hip, kwage_group_union_columns): new
// columns of a RESIDENT matrix, each the OR of listed columns of a resident matrix (the same one or another).
#ifndef KWAGE_AMD_UNION_KERNELS_HPP
#define KWAGE_AMD_UNION_KERNELS_HPP

#include "union_plan.hpp"

namespace kwage {

constexpr int UNION_THREADS = 256;

// union_columns_kernel: in every row of `dst` the units [first_unit, first_unit + units) are stored -- destination column
// first_column + j is set where any member of set j is set in the same row of `src` (union_plan.hpp union_unit_value),
// zero at and above first_column + n up to the end of the 32-bit word that holds the last column: what the live insert
// owns, so that the matrix is the insert's bit for bit up to the stride.  `src` and `dst` have the same number of rows.
//
// Ownership: one lane per (destination row, 16-byte unit), consecutive lanes consecutive units of a row.  A lane makes its
// unit in registers and stores it with ONE 16-byte store -- every byte is written once, by one lane: no atomics, no LDS,
// nothing cleared beforehand.  The destination is read only for what a unit keeps (copy_plan.hpp copy_keep_mask), by the
// owners of a row's first and last unit, and that read is requested before the source loads.
//
// `src` and `dst` may be the SAME matrix: the plan then places the new columns at a 16-byte boundary of the row at or above
// the span, so every unit written lies wholly above every member, and what the last unit keeps is read through `dst` from
// the bytes this very lane stores -- no byte that is written is read through `src`, by any lane: no ordering is needed
// and both __restrict__ hold.
//
// A lane walks the entries of its up to 128 sets as one stretch of the table, UNION_LOADS at a time: the entries (16
// bytes each, read alike by every lane that owns this unit in another row: they stay cached), then their source dwords
// together.  Plain loads: a source line serves the lane's later entries and the neighbouring rows' lanes.  All offsets in
// 64 bits.
__global__ __launch_bounds__(UNION_THREADS) void union_columns_kernel(
	const uint8_t *__restrict__ src, uint64_t src_stride, uint8_t *__restrict__ dst, uint64_t dst_stride, uint64_t nrows,
	const UnionEntry *__restrict__ entries, const uint32_t *__restrict__ offsets,      // the plan: union_plan.hpp UnionPlan
	uint64_t first_column, uint64_t n, uint64_t first_unit, uint64_t units)
{
	const uint64_t total = nrows*units;
	auto entry = [&](uint64_t i) {
		const uint4 q = *reinterpret_cast<const uint4*>(entries + i);
		return UnionEntry{q.x, q.y, q.z, q.w};
	};
	auto load = [&](uint64_t byte) { return *reinterpret_cast<const uint32_t*>(src + byte); };
	const uint64_t last_unit = first_unit + units - 1;
	const bool keeps_low = first_column % 128 != 0, keeps_high = ((first_column + n - 1)/32) % 4 != 3;
	for(uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x*blockDim.x){
		const uint64_t row = (i >> 32) == 0 ? (uint32_t)i/(uint32_t)units : i/units;
		const uint64_t unit = first_unit + (i - row*units);
		uint4 *out = reinterpret_cast<uint4*>(dst + row*dst_stride + 16*unit);
		const bool reads = (keeps_low && unit == first_unit) || (keeps_high && unit == last_unit);
		uint4 old = make_uint4(0u, 0u, 0u, 0u);
		if(reads){ old = *out; }
		uint32_t w[4];
		union_unit_value(entry, load, offsets, row, src_stride, first_column, n, unit, w);
		if(reads){
			uint32_t keep[4];
			copy_keep_mask(first_column, n, unit, keep);
			w[0] |= old.x & keep[0]; w[1] |= old.y & keep[1]; w[2] |= old.z & keep[2]; w[3] |= old.w & keep[3];
		}
		*out = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

}  // namespace kwage

#endif
