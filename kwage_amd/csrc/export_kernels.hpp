// kwage_amd/csrc/export_kernels.hpp -- the kernel of the export (export.hip, kwage_group_export_filters): listed columns of
// the RESIDENT row-major matrix become whole Bloom filters again -- filter-major, LSB first, the payload of a `.bloom`
// file.  The live insert's kernel (insert_kernels.hpp) run backwards on the same tile (transpose_tile.hpp), its column
// gathering the save's (save_plan.hpp).
#ifndef KWAGE_AMD_EXPORT_KERNELS_HPP
#define KWAGE_AMD_EXPORT_KERNELS_HPP

#include "export_plan.hpp"
#include "transpose_tile.hpp"

namespace kwage {

typedef uint32_t export_v4 __attribute__((ext_vector_type(4)));      // 16 bytes as a clang vector: the nontemporal builtins take it

// export_filters_kernel: rows row_base .. row_base + chunk_rows - 1 of the n listed columns (the plan's runs: destination =
// filter index, source = column) become chunk_rows bits of n filters, filter f at out + f*out_stride, its byte b the rows
// row_base + 8b .. row_base + 8b + 7.  Exactly ceil(chunk_rows / 8) bytes of every filter are written; rows beyond the
// chunk are zero bits of a filter's last byte (filters of fewer than 8 rows).
//
// A tile is TransposeTile's: ROWS rows x PITCH words of 32 listed filters each; a workgroup makes one.
//
// Load phase: the tile is filled in LDS as the save's extract kernel fills an output row, one 16-byte unit (four words =
// 128 listed filters) per thread and step: a unit wholly inside one run takes save_unit_in_run (one 16-byte load where the
// run is aligned, else four dword loads and a fifth, requested together), any other unit is walked word by word with
// save_word; filters at and above n are zero bits.  Every source byte is used once: nontemporal loads.  LDS columns are
// rotated by 16 bytes per 32 rows, as in the insert, so that the reads of phase two spread over the banks.
//
// Transpose-and-store phase: lane (g, d) reads tile[32d + b][g], b = 0 .. 31, transposes the 32 x 32 block in registers
// and stores register i as the dword of rows 32d .. 32d + 31 of filter 32(g0 + g) + i: LD consecutive lanes write
// consecutive dwords of one filter.  Where the tile's whole row range exists and dwords are aligned (uniform over the
// workgroup) a group of 32 existing filters is 32 dword stores with no branch between them; the last rows of a chunk and
// filters shorter than a dword go byte by byte.  A group of 32 filters that does not exist is neither read from LDS nor
// transposed nor stored.
//
// Ownership: one thread owns an (output filter, dword): no atomics, no read of the output, nothing to clear beforehand.
// The matrix is only read.
template<int LD, int TB_WAVES>
__global__ __launch_bounds__(TB_WAVES*64) void export_filters_kernel(
	const uint8_t *__restrict__ matrix, uint64_t stride, uint64_t matrix_bytes,
	const SaveRun *__restrict__ runs, uint32_t n_runs, uint32_t n,        // the plan; n filters
	uint64_t row_base, uint64_t chunk_rows,                               // the chunk's rows
	uint8_t *__restrict__ out, uint64_t out_stride,
	uint32_t tiles_x)                                                     // row tiles per filter tile
{
	using T = TransposeTile<LD, TB_WAVES>;
	__shared__ uint32_t tile[T::ROWS*T::PITCH];
	constexpr uint32_t SEGS = T::PITCH/4;                     // 16-byte units per row of the tile

	const uint64_t row0 = (uint64_t)(blockIdx.x % tiles_x)*T::ROWS;      // first row of the tile within the chunk
	const uint64_t f0 = (uint64_t)(blockIdx.x / tiles_x)*T::FILTERS;     // first listed filter of the tile
	if(row0 >= chunk_rows || f0 >= n){ return; }
	const uint64_t tile_rows = std::min<uint64_t>(T::ROWS, chunk_rows - row0);
	const uint32_t fill_rows = (uint32_t)((tile_rows + 31)/32*32);       // rows phase two reads: whole blocks of 32

	// load phase
	for(uint32_t i = threadIdx.x; i < fill_rows*SEGS; i += TB_WAVES*64){
		const uint32_t r = i / SEGS, seg = i % SEGS;
		const uint64_t d0 = f0 + 128ull*seg;                  // first listed filter of the unit
		if(d0 >= n){ continue; }                              // (its groups do not exist: never read)
		uint32_t w[4] = {0u, 0u, 0u, 0u};
		if(r < tile_rows){
			const uint64_t row = row_base + row0 + r;
			uint32_t k = save_find_run(runs, n_runs, (uint32_t)d0);
			const SaveRun first = runs[k];
			if(d0 + 128 <= (uint64_t)first.dst_first + first.len){
				// the whole unit inside one run: its loads in flight together
				auto load = [&](uint64_t byte) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(matrix + byte)); };
				auto load4 = [&](uint64_t byte) {
					const export_v4 q = __builtin_nontemporal_load(reinterpret_cast<const export_v4*>(matrix + byte));
					return SaveQuad{q.x, q.y, q.z, q.w};
				};
				save_unit_in_run(load, load4, row, stride, first.src_first + ((uint32_t)d0 - first.dst_first), w);
			}
			else{
				// a unit that runs end or begin in, or the list's last one: piece by piece, the dword loaded last kept
				uint64_t have_byte = ~0ull;
				uint32_t have = 0;
				auto load = [&](uint64_t byte) {
					if(byte != have_byte){
						have = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(matrix + byte));
						have_byte = byte;
					}
					return have;
				};
#pragma unroll
				for(int j = 0; j < 4; ++j){
					const uint64_t b = d0 + 32u*j;
					w[j] = b < n ? save_word(load, runs, &k, row, stride, matrix_bytes, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + 32, n)) : 0u;
				}
			}
		}
		*reinterpret_cast<uint4*>(&tile[r*T::PITCH + 4*((seg + r/32) % SEGS)]) = make_uint4(w[0], w[1], w[2], w[3]);
	}
	__syncthreads();

	// transpose-and-store phase
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = threadIdx.x >> 6;
	const uint32_t d = lane % LD;                             // dword of the tile's row range
	const uint32_t g = wave*(64/LD) + lane/LD;                // group of 32 listed filters of the tile
	const uint64_t first = f0 + 32ull*g;                      // its first filter
	const uint64_t tile_bytes = (chunk_rows - row0 + 7)/8;    // bytes of a filter left in the chunk from the tile's first row on
	if(first >= n || 4ull*d >= tile_bytes){ return; }

	uint32_t a[32];
	const uint32_t col = (g + 4*d) % T::PITCH;                // rotation: 4 dwords (16 bytes) per 32 rows
#pragma unroll
	for(int b = 0; b < 32; ++b){ a[b] = tile[(32*d + b)*T::PITCH + col]; }
	transpose_32x32(a);

	uint8_t *dst = out + first*out_stride + row0/8 + 4*d;
	const uint32_t count = (uint32_t)std::min<uint64_t>(32, n - first);      // filters of the group that exist
	if(tile_bytes >= 4ull*LD && (out_stride & 3) == 0 && (((uintptr_t)out) & 3) == 0){
		// the whole row range of the tile exists and dwords are aligned (uniform over the workgroup)
		if(count == 32){
#pragma unroll
			for(int i = 0; i < 32; ++i){ *reinterpret_cast<uint32_t*>(dst + (uint64_t)i*out_stride) = a[i]; }
		}
		else{
#pragma unroll
			for(int i = 0; i < 32; ++i){ if((uint32_t)i < count){ *reinterpret_cast<uint32_t*>(dst + (uint64_t)i*out_stride) = a[i]; } }
		}
	}
	else{
		// the last rows of a chunk, or filters shorter than a dword: byte by byte
		const uint32_t have = (uint32_t)std::min<uint64_t>(4, tile_bytes - 4ull*d);
#pragma unroll
		for(int i = 0; i < 32; ++i){
			if((uint32_t)i >= count){ continue; }
#pragma unroll
			for(uint32_t b = 0; b < 4; ++b){ if(b < have){ dst[(uint64_t)i*out_stride + b] = (uint8_t)(a[i] >> (8*b)); } }
		}
	}
}

}  // namespace kwage

#endif
