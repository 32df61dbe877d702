// kwage_amd/csrc/save_kernels.hpp -- the kernel of the save (save.hip, kwage_group_save_db): chosen columns of the
// RESIDENT row-major matrix gathered and packed densely, as the body of a `.db` file.
#ifndef KWAGE_AMD_SAVE_KERNELS_HPP
#define KWAGE_AMD_SAVE_KERNELS_HPP

#include "save_plan.hpp"

namespace kwage {

typedef uint32_t save_v4 __attribute__((ext_vector_type(4)));      // 16 bytes as a clang vector: the nontemporal builtins take it

// extract_columns_kernel: rows r0 .. r0 + nr - 1 of the matrix (rows `stride` bytes apart, matrix_bytes in all) become nr
// rows of out_slice = ceil(n / 8) bytes in `out`, the file's body for those rows exactly: no padding between rows, LSB
// first, destination column d = source column of the run that covers d (save_plan.hpp), the bits at and above n in a
// row's last byte zero.
//
// Ownership: a thread makes one 16-byte unit (128 destination columns) of one row, four words one after the other, and
// stores it -- every output byte is written exactly once, by one thread: no atomics, and nothing has to be cleared
// beforehand.  STORE is the widest store the layout allows: 16 where out_slice % 16 == 0 (every unit is whole and 16-byte
// aligned: one store per thread), 4 where out_slice % 4 == 0 (the last unit of a row may be short, by whole dwords), else
// 1 (row starts lie off dword boundaries: byte stores).
//
// Gathering: the run that covers a unit's first column is found by binary search of the run table (as run_copy in
// hit_sort.hip finds its first run), the thread then walks on through the runs.  A piece of a word is a funnel shift over
// two aligned source dwords (save_piece), the dword loaded last kept for the next piece.  A unit that lies inside ONE run
// -- all but the units at run ends -- takes no walk: its four source dwords (one 16-byte load where they start on a
// 16-byte boundary, as the columns of a file block saved from its start do) and a fifth where the columns start off a dword
// boundary are requested together (save_unit_in_run).  Every source byte is used once: nontemporal loads, as in the
// gather kernels.
template<int STORE>
__global__ __launch_bounds__(256) void extract_columns_kernel(
	const uint8_t *__restrict__ matrix, uint64_t stride, uint64_t matrix_bytes,
	const SaveRun *__restrict__ runs, uint32_t n_runs, uint32_t n,        // the plan; n destination columns
	uint64_t r0, uint64_t nr,                                             // the chunk's rows
	uint8_t *__restrict__ out, uint64_t out_slice)
{
	const uint64_t units = (out_slice + 15)/16;                           // 16-byte units of an output row
	const uint64_t total = nr*units;
	for(uint64_t i = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x*blockDim.x){
		const uint64_t r = i / units, u = i % units;
		const uint64_t row = r0 + r;
		const uint32_t d0 = (uint32_t)(128*u);                            // (u < 2^25: n < 2^32)
		uint32_t k = save_find_run(runs, n_runs, d0);
		const SaveRun first = runs[k];
		uint32_t w[4];
		if((uint64_t)d0 + 128 <= (uint64_t)first.dst_first + first.len){
			// the whole unit inside one run (the common case: long runs): its loads in flight together
			auto load = [&](uint64_t byte) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(matrix + byte)); };
			auto load4 = [&](uint64_t byte) {
				const save_v4 q = __builtin_nontemporal_load(reinterpret_cast<const save_v4*>(matrix + byte));
				return SaveQuad{q.x, q.y, q.z, q.w};
			};
			save_unit_in_run(load, load4, row, stride, first.src_first + (d0 - first.dst_first), w);
		}
		else{
			// a unit that runs end or begin in, or a row's last one: piece by piece, the dword loaded last kept
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
				const uint64_t b = (uint64_t)d0 + 32u*j;                  // (64 bits: d0 + 96 may pass 2^32)
				w[j] = b < n ? save_word(load, runs, &k, row, stride, matrix_bytes, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + 32, n)) : 0u;
			}
		}
		uint8_t *dst = out + r*out_slice + 16*u;
		if(STORE == 16){
			*reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
		}
		else if(STORE == 4){
			const uint32_t words = (uint32_t)std::min<uint64_t>(4, (out_slice - 16*u)/4);
#pragma unroll
			for(uint32_t j = 0; j < 4; ++j){ if(j < words){ reinterpret_cast<uint32_t*>(dst)[j] = w[j]; } }
		}
		else{
			const uint32_t bytes = (uint32_t)std::min<uint64_t>(16, out_slice - 16*u);
#pragma unroll
			for(uint32_t j = 0; j < 16; ++j){ if(j < bytes){ dst[j] = (uint8_t)(w[j/4] >> (8*(j%4))); } }
		}
	}
}

}  // namespace kwage

#endif
