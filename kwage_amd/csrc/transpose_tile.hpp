// kwage_amd/csrc/transpose_tile.hpp -- the 32 x 32 bit transpose in registers and the tile it works on: what the database
// builder (builder.hip, transpose_bits_kernel: filters in, a packed slice block out) and the live insert
// (insert_kernels.hpp, insert_filters_kernel: filters in, new columns of a resident matrix out) share.  Device code only.
#ifndef KWAGE_AMD_TRANSPOSE_TILE_HPP
#define KWAGE_AMD_TRANSPOSE_TILE_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace kwage {

// One workgroup = 8 waves = a tile of FILTERS filters x ROWS slices (TransposeTile: 64 KB in, 64 KB out).
//
// A lane holds a 32 x 32 bit block: one dword (32 consecutive slices) of each of 32 consecutive filters, loaded so
// that LD consecutive lanes read consecutive dwords of the same filter (64- or 128-byte runs per filter), transposes
// it in registers (five rounds of masked half-block swaps, ~480 integer operations for 1024 bits -- the ballot form
// this replaces spent five instructions per 64 bits and was VALU-bound at 0.15 of the HBM rate) and leaves 32 dwords
// in LDS: slice (32d + b), the four bytes of its 32 filters.  The tile is then written out as whole row segments of
// FILTERS/8 bytes, 16 bytes per thread.  LDS columns are rotated by 16 bytes per 32 slices so that the lanes of
// one store spread over the banks (rows are FILTERS/8 = 128 or 64 bytes apart).
template<int LD, int TB_WAVES> struct TransposeTile {
	static constexpr int WAVES = TB_WAVES;
	static constexpr int ROWS = 32*LD;                        // slices per tile
	static constexpr int GROUPS = TB_WAVES*(64/LD);           // 32-filter groups per tile
	static constexpr int FILTERS = 32*GROUPS;
	static constexpr int PITCH = GROUPS;                      // dwords per LDS row
	static_assert(ROWS*PITCH*4 == TB_WAVES*8*1024, "8 KB per wave");
};

__device__ inline void transpose_32x32(uint32_t (&a)[32])
{
	// a[i] bit b  <->  a[b] bit i (both LSB-first)
#pragma unroll
	for(int s = 0; s < 5; ++s){
		const int j = 16 >> s;
		const uint32_t m = s == 0 ? 0x0000FFFFu : s == 1 ? 0x00FF00FFu : s == 2 ? 0x0F0F0F0Fu : s == 3 ? 0x33333333u : 0x55555555u;
#pragma unroll
		for(int k = 0; k < 32; ++k){
			if(k & j){ continue; }
			const uint32_t t = ((a[k] >> j) ^ a[k + j]) & m;
			a[k + j] ^= t;
			a[k] ^= t << j;
		}
	}
}

// A lane's 32 dwords of tile (row0, f0): the loads are ISSUED here and nothing else touches the values on the fast path
// (filters past the last one read the last one's dword; tile_zero_past_end() clears them before the transpose), so the
// caller can leave them in flight behind other work.
template<int LD>
__device__ __forceinline__ void tile_request(uint32_t (&a)[32], const uint8_t *__restrict__ in, uint64_t in_stride, uint32_t n_filters,
                                             uint64_t chunk_rows, uint64_t row0, uint32_t first, uint32_t d)
{
	const uint64_t tile_bytes = (chunk_rows - row0 + 7)/8;    // bytes of a filter left in the chunk from the tile's first slice on
	if(tile_bytes >= 4ull*LD && (in_stride & 3) == 0 && (((uintptr_t)in) & 3) == 0){
		// the whole row range of the tile exists and dwords are aligned (uniform over the workgroup): 32 loads in flight
		// per lane, no branch between them
		const uint32_t last = first < n_filters ? std::min<uint32_t>(31u, n_filters - 1 - first) : 0u;
		const uint8_t *base = in + (uint64_t)(first < n_filters ? first : 0u)*in_stride + row0/8 + 4*d;
#pragma unroll
		for(int i = 0; i < 32; ++i){
			a[i] = *reinterpret_cast<const uint32_t*>(base + (uint64_t)std::min<uint32_t>((uint32_t)i, last)*in_stride);
		}
	}
	else{
		// the last rows of a chunk, or filters shorter than a dword: byte by byte
		const uint32_t have = tile_bytes > 4ull*d ? (uint32_t)std::min<uint64_t>(4, tile_bytes - 4ull*d) : 0;
#pragma unroll 1
		for(int i = 0; i < 32; ++i){
			const uint32_t f = first + i;
			uint32_t v = 0;
			if(f < n_filters){
				const uint8_t *src = in + (uint64_t)f*in_stride + row0/8 + 4*d;
				for(uint32_t b = 0; b < have; ++b){ v |= (uint32_t)src[b] << (8*b); }
			}
			a[i] = v;
		}
	}
}

__device__ __forceinline__ void tile_zero_past_end(uint32_t (&a)[32], uint32_t first, uint32_t n_filters)
{
#pragma unroll
	for(int i = 0; i < 32; ++i){ a[i] = first + i < n_filters ? a[i] : 0u; }
}

}  // namespace kwage

#endif
