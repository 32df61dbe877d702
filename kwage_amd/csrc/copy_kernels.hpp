// kwage_amd/csrc/copy_kernels.hpp -- the kernel of the copy between groups (copy.hip, kwage_group_copy_columns): listed
// columns of one RESIDENT matrix packed densely into another one's rows at a bit offset.
#ifndef KWAGE_AMD_COPY_KERNELS_HPP
#define KWAGE_AMD_COPY_KERNELS_HPP

#include "copy_plan.hpp"

namespace kwage {

typedef uint32_t copy_v4 __attribute__((ext_vector_type(4)));      // 16 bytes as a clang vector: the nontemporal builtins take it

constexpr int COPY_THREADS = 256;

// copy_columns_kernel: in every row of `dst` the units [first_unit, first_unit + units) are stored -- destination column
// first_column + d = the source column of the run that covers d (copy_plan.hpp copy_unit_value), zero at and above
// first_column + n up to the end of the 32-bit word that holds the last column: what the live insert owns, so that the
// matrix is the insert's bit for bit up to the stride.  `src` and `dst` are different allocations with the same number
// of rows.
//
// Ownership: one lane per (destination row, 16-byte unit), consecutive lanes consecutive units of a row, so a wave's loads
// of a source row and its stores are contiguous wherever a row has 64 units to write.  A lane makes its unit in registers
// and stores it with ONE 16-byte store (the stride is a multiple of 128: every unit is whole and aligned) -- every byte
// is written once, by one lane: no atomics, no LDS, nothing cleared beforehand.  The destination is read only for what a
// unit keeps (copy_plan.hpp copy_keep_mask): by the owner of a row's first unit where first_column % 128 != 0, for the
// bits below first_column, and by the owner of its last unit where the last word written is not the unit's last, for
// the words above it -- two lanes per row at the most, one where the copy stays within a unit.
//
// A unit wholly inside the copied columns and inside one run -- all but a row's first and last and those at run ends --
// has its four or five source dwords requested together: one 16-byte load (and a dword) where they start on a 16-byte
// boundary of the row, else the two aligned 16-byte pieces that hold them (copy_plan.hpp copy_unit_off_boundary).  Every
// source byte is used once or twice (what two units share): nontemporal loads, as in extract_columns_kernel.  All
// offsets in 64 bits.
__global__ __launch_bounds__(COPY_THREADS) void copy_columns_kernel(
	const uint8_t *__restrict__ src, uint64_t src_stride, uint8_t *__restrict__ dst, uint64_t dst_stride, uint64_t nrows,
	const SaveRun *__restrict__ runs, uint32_t n_runs,                     // the plan: copy_plan.hpp CopyPlan
	uint64_t first_column, uint64_t n, uint64_t first_unit, uint64_t units)
{
	const uint64_t src_bytes = nrows*src_stride, total = nrows*units;
	auto load = [&](uint64_t byte) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + byte)); };
	auto load4 = [&](uint64_t byte) {
		const copy_v4 q = __builtin_nontemporal_load(reinterpret_cast<const copy_v4*>(src + byte));
		return SaveQuad{q.x, q.y, q.z, q.w};
	};
	const uint64_t last_unit = first_unit + units - 1;
	const bool keeps_low = first_column % 128 != 0, keeps_high = ((first_column + n - 1)/32) % 4 != 3;
	for(uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x*blockDim.x){
		// (one division, of 32-bit values wherever the item number has 32 bits: units is below 2^32)
		const uint64_t row = (i >> 32) == 0 ? (uint32_t)i/(uint32_t)units : i/units;
		const uint64_t unit = first_unit + (i - row*units);
		uint4 *out = reinterpret_cast<uint4*>(dst + row*dst_stride + 16*unit);
		// what the unit keeps is requested BEFORE the source: one lane's second round trip would otherwise be its whole wave's
		// (profiles/r12_copy_bench.txt, case b)
		const bool reads = (keeps_low && unit == first_unit) || (keeps_high && unit == last_unit);
		uint4 old = make_uint4(0u, 0u, 0u, 0u);
		if(reads){ old = *out; }
		uint32_t w[4];
		copy_unit_value(load, load4, runs, n_runs, row, src_stride, src_bytes, first_column, n, unit, w);
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
