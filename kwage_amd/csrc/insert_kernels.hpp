// kwage_amd/csrc/insert_kernels.hpp -- the kernels of the live insert (insert.hip): whole Bloom filters become new
// columns of a RESIDENT row-major matrix, and withdrawn columns are cleared.  The tile, its loads and the 32 x 32 bit
// transpose in registers are the database builder's (transpose_tile.hpp); what differs is where the tile goes.
#ifndef KWAGE_AMD_INSERT_KERNELS_HPP
#define KWAGE_AMD_INSERT_KERNELS_HPP

#include "insert_plan.hpp"
#include "transpose_tile.hpp"

namespace kwage {

// insert_filters_kernel: n filters (in: [n][in_stride bytes], chunk_rows bits of each, LSB first) become columns
// first_column .. first_column + n - 1 of rows row_base .. row_base + chunk_rows - 1 of the matrix (rows `stride` bytes apart).
//
// A tile is TransposeTile's: ROWS rows x PITCH destination words of 32 columns, and the tiles of a row start at word
// word_base, the 16-byte boundary at or below the insert's first word, so that every 16-byte segment of a tile is a
// 16-byte aligned piece of a matrix row.  The insert's BIT OFFSET is taken on the load side: destination column
// 32*word_base + v holds filter v - shift (shift = first_column - 32*word_base, 0 .. 127), so a lane whose 32 x 32 block
// covers destination columns v0 .. v0 + 31 loads filters v0 - shift .. v0 + 31 - shift into registers 0 .. 31 -- registers
// whose filter does not exist hold zero -- and the transposed block IS 32 rows of one destination word: no word is put
// together from two transposed words, and no workgroup needs a filter group of its neighbour's.  A block none of whose
// filters exists is not loaded, transposed or left in LDS at all (an insert of one filter loads one block per 32 rows).
//
// Ownership: the call owns words word_first .. word_last of every row, one thread per (row, word); of word_first the
// bits below keep_bits (columns of earlier inserts) are kept from memory -- the only load of the matrix -- and everything
// at and above the new tail is written as zero.  Nothing else of a row is touched: no atomics.  Segments that lie
// wholly inside the owned words are stored 16 bytes per thread, the first and last segment of a row word by word.
template<int LD>
__device__ __forceinline__ bool insert_tile_request(uint32_t (&a)[32], const uint8_t *__restrict__ in, uint64_t in_stride, uint32_t n_filters,
                                                    uint32_t shift, uint64_t chunk_rows, uint64_t row0, uint64_t v0, uint32_t d)
{
	// destination columns (relative to 32*word_base) that hold a filter: [shift, shift + n_filters)
	const uint64_t lo = std::max<uint64_t>(v0, shift), hi = std::min<uint64_t>(v0 + 32, (uint64_t)shift + n_filters);
	if(lo >= hi){ return false; }
	const uint32_t ilo = (uint32_t)(lo - v0), ihi = (uint32_t)(hi - 1 - v0);      // registers that hold a filter
	const uint64_t tile_bytes = (chunk_rows - row0 + 7)/8;    // bytes of a filter left in the chunk from the tile's first row on
	if(tile_bytes >= 4ull*LD && (in_stride & 3) == 0 && (((uintptr_t)in) & 3) == 0){
		// the whole row range of the tile exists and dwords are aligned (uniform over the workgroup): 32 loads in flight per
		// lane; registers outside [ilo, ihi] read a neighbour's dword and are cleared below
		const uint8_t *base = in + (v0 - shift + ilo)*in_stride + row0/8 + 4*d;      // filter of register ilo (v0 + ilo >= shift)
#pragma unroll
		for(int i = 0; i < 32; ++i){
			const uint32_t c = std::min<uint32_t>(std::max<uint32_t>((uint32_t)i, ilo), ihi) - ilo;
			a[i] = *reinterpret_cast<const uint32_t*>(base + (uint64_t)c*in_stride);
		}
#pragma unroll
		for(int i = 0; i < 32; ++i){ a[i] = ((uint32_t)i >= ilo && (uint32_t)i <= ihi) ? a[i] : 0u; }
	}
	else{
		// the last rows of a chunk, or filters shorter than a dword: byte by byte
		const uint32_t have = tile_bytes > 4ull*d ? (uint32_t)std::min<uint64_t>(4, tile_bytes - 4ull*d) : 0;
#pragma unroll 1
		for(int i = 0; i < 32; ++i){
			uint32_t v = 0;
			if((uint32_t)i >= ilo && (uint32_t)i <= ihi){
				const uint8_t *src = in + (v0 + i - shift)*in_stride + row0/8 + 4*d;
				for(uint32_t b = 0; b < have; ++b){ v |= (uint32_t)src[b] << (8*b); }
			}
			a[i] = v;
		}
	}
	return true;
}

template<int LD, int TB_WAVES>
__global__ __launch_bounds__(TB_WAVES*64) void insert_filters_kernel(
	const uint8_t *__restrict__ in, uint64_t in_stride,   // [n_filters][in_stride bytes]: this chunk's bits
	uint32_t n_filters, uint64_t chunk_rows,              // rows in this chunk
	uint8_t *matrix, uint64_t stride, uint64_t row_base,  // the group's matrix; its row of the chunk's first row
	uint64_t word_base, uint64_t word_first, uint64_t word_last, uint32_t keep_bits, uint32_t shift,      // insert_plan.hpp InsertSpan
	uint32_t tiles_x)                                     // row tiles per column tile
{
	using T = TransposeTile<LD, TB_WAVES>;
	__shared__ uint32_t tile[T::ROWS*T::PITCH];

	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = threadIdx.x >> 6;
	const uint32_t d = lane % LD;                             // dword of the tile's row range
	const uint32_t g = wave*(64/LD) + lane/LD;                // destination word of the tile
	constexpr uint32_t SEGS = T::PITCH/4;                     // 16-byte segments per row of the tile

	const uint64_t row0 = (uint64_t)(blockIdx.x % tiles_x)*T::ROWS;
	const uint64_t w0 = word_base + (uint64_t)(blockIdx.x / tiles_x)*T::PITCH;       // first destination word of the tile
	if(row0 >= chunk_rows || w0 > word_last){ return; }

	uint32_t a[32];
	if(insert_tile_request<LD>(a, in, in_stride, n_filters, shift, chunk_rows, row0, 32*(w0 - word_base + g), d)){
		transpose_32x32(a);
		const uint32_t col = (g + 4*d) % T::PITCH;            // rotation: 4 dwords (16 bytes) per 32 rows
#pragma unroll
		for(int b = 0; b < 32; ++b){ tile[(32*d + b)*T::PITCH + col] = a[b]; }
	}
	__syncthreads();

	// write the tile: ROWS rows x PITCH words; a thread moves 16 bytes.  (Words of blocks that were not loaded lie outside
	// [word_first, word_last]: what LDS holds for them is never stored.)
	const uint32_t keep = keep_bits ? (1u << keep_bits) - 1 : 0u;
	for(uint32_t i = threadIdx.x; i < T::ROWS*SEGS; i += TB_WAVES*64){
		const uint32_t r = i / SEGS, seg = i % SEGS;
		if(row0 + r >= chunk_rows){ continue; }
		const uint64_t w = w0 + 4*seg;                        // first word of the segment
		if(w + 3 < word_first || w > word_last){ continue; }
		uint32_t *dst = reinterpret_cast<uint32_t*>(matrix + (row_base + row0 + r)*stride) + w;
		const uint4 v = *reinterpret_cast<const uint4*>(&tile[r*T::PITCH + 4*((seg + r/32) % SEGS)]);
		if(w + 3 <= word_last && (w > word_first || (w == word_first && keep == 0))){ *reinterpret_cast<uint4*>(dst) = v; }
		else{
			const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for(uint32_t k = 0; k < 4; ++k){
				if(w + k < word_first || w + k > word_last){ continue; }
				dst[k] = (w + k == word_first && keep) ? ((dst[k] & keep) | x[k]) : x[k];
			}
		}
	}
}

// retire_columns_kernel: one thread per (row, pair) clears the pair's mask in its word of the row.  The pairs of a call
// name distinct words (insert_plan.hpp plan_retire), so no two threads meet in a word.
__global__ void retire_columns_kernel(uint8_t *matrix, uint64_t stride, uint64_t nrows, const RetirePair *__restrict__ pairs, uint64_t n_pairs)
{
	const uint64_t total = nrows*n_pairs;
	for(uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x*blockDim.x){
		const uint64_t r = i / n_pairs;
		const RetirePair p = pairs[i % n_pairs];
		uint32_t *w = reinterpret_cast<uint32_t*>(matrix + r*stride) + p.word;
		*w &= ~p.mask;
	}
}

}  // namespace kwage

#endif
