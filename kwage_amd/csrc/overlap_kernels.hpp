// kwage_amd/csrc/overlap_kernels.hpp -- the kernels of the overlap matrix (overlap.hip, kwage_group_column_overlaps): the
// shared set bits of every pair of listed columns of two RESIDENT matrices, as the integer matrix product it is, on the
// matrix cores.
#ifndef KWAGE_AMD_OVERLAP_KERNELS_HPP
#define KWAGE_AMD_OVERLAP_KERNELS_HPP

#include "overlap_plan.hpp"
#include "transpose_tile.hpp"

namespace kwage {

constexpr int OVERLAP_THREADS = 256;
// LDS image of a step: [8 blocks][32 groups of rows][32 columns] words, a group's 32 words 33 apart -- the lanes of a
// half wave, which write the same column of 32 different groups, and the lanes that read 32 columns of one group both
// spread over the banks.
constexpr uint32_t OVERLAP_LDS_PITCH = OVERLAP_BLOCK + 1;
constexpr uint32_t OVERLAP_LDS_BLOCK = OVERLAP_STEP_GROUPS*OVERLAP_LDS_PITCH;

typedef int overlap_v4i __attribute__((ext_vector_type(4)));
typedef int overlap_v16i __attribute__((ext_vector_type(16)));

// Cell (ia, jb) of the result, and in the symmetric form its mirror for a tile above the diagonal: one store each, by
// the one lane that holds the sum.
__device__ __forceinline__ void overlap_store_cell(const OverlapArgs &p, bool mirror, uint64_t ia, uint64_t jb, uint32_t v)
{
	if(ia < p.n_a && jb < p.n_b){
		p.cells[ia*p.row_elems + jb] = v;
		if(mirror){ p.cells[jb*p.row_elems + ia] = v; }
	}
}

// overlap_mfma_kernel: workgroup (tile, part) sums, over the rows of its part, the products of the tile's 128 columns of
// `a` with its 128 columns of `b` -- cell (i, j) = the number of rows in which both are set.
//
// A step is 32 groups of 32 rows.  Staging: lane (block, group) -- eight blocks, four of either side -- makes the 32
// words "32 rows of one column" of its block and group.  Straight block: the row dwords of the group (32 loads in
// flight), ANDed with the block's mask, transposed in registers (transpose_tile.hpp).  Gathered block: column after
// column the row dwords that hold it (loaded again only where the dword changes) and the column's bit of each.  The words
// go to LDS.  Product: wave (wm, wn) owns the 64 x 64 quarter of the tile as 2 x 2 accumulator blocks; per group of rows a
// lane reads the words of its column of two blocks of either side, spreads its half of each into 16 bytes of 0 / 1
// (overlap_plan.hpp overlap_spread) and issues four v_mfma_i32_32x32x32_i8.  Integer sums: exact, in any order, up to
// 2^31 rows; no floating point anywhere.
//
// Ownership: accumulator register `reg` of lane (r, h) is cell (row (reg & 3) + 8 (reg >> 2) + 4 h, column r) of its
// block; every cell (or partial cell) is stored once by that lane, no atomics, nothing cleared beforehand.  With one part
// the cells go to the result, else to the part's partial tile, which overlap_combine_kernel sums.
__global__ __launch_bounds__(OVERLAP_THREADS) void overlap_mfma_kernel(OverlapArgs p)
{
	__shared__ uint32_t lds[2*OVERLAP_TILE_BLOCKS*OVERLAP_LDS_BLOCK];
	const uint32_t tile = blockIdx.x % p.n_tiles, part = blockIdx.x / p.n_tiles;
	const OverlapTile tl = p.tiles[tile];
	const uint64_t g_begin = overlap_part_begin(p.groups, p.splits, part), g_end = overlap_part_begin(p.groups, p.splits, part + 1);

	// staging role
	const uint32_t sblock = threadIdx.x >> 5, sgroup = threadIdx.x & 31;
	const bool side_b = sblock >= OVERLAP_TILE_BLOCKS;
	const uint32_t bi = (side_b ? tl.tb : tl.ta)*OVERLAP_TILE_BLOCKS + (sblock & (OVERLAP_TILE_BLOCKS - 1));
	const bool have = bi < (side_b ? p.n_blocks_b : p.n_blocks_a);
	const OverlapBlock *blk = (side_b ? p.blocks_b : p.blocks_a) + (have ? bi : 0u);
	const uint8_t *bits = side_b ? p.b_bits : p.a_bits;
	const uint64_t stride = side_b ? p.b_stride : p.a_stride;
	const bool straight = blk->straight != 0;
	const uint32_t s_dword = blk->dword, s_mask = blk->mask;
	uint32_t *stage = lds + sblock*OVERLAP_LDS_BLOCK + sgroup*OVERLAP_LDS_PITCH;
	auto load = [&](uint64_t byte) { return *reinterpret_cast<const uint32_t*>(bits + byte); };

	// product role
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
	const uint32_t *frag_a = lds + (2*wm)*OVERLAP_LDS_BLOCK + r, *frag_b = lds + (OVERLAP_TILE_BLOCKS + 2*wn)*OVERLAP_LDS_BLOCK + r;
	overlap_v16i acc[2][2];
#pragma unroll
	for(int i = 0; i < 2; ++i){
#pragma unroll
		for(int j = 0; j < 2; ++j){
#pragma unroll
			for(int k = 0; k < 16; ++k){ acc[i][j][k] = 0; }
		}
	}

	for(uint64_t g0 = g_begin; g0 < g_end; g0 += OVERLAP_STEP_GROUPS){
		const uint64_t group = g0 + sgroup;
		const uint64_t first_row = group*32, end_row = group < g_end ? (uint64_t)p.rows : 0;
		uint32_t v[32];
		if(!have){
#pragma unroll
			for(int c = 0; c < 32; ++c){ stage[c] = 0u; }
		}
		else if(straight){
			overlap_stage_rows(load, stride, s_dword, s_mask, first_row, end_row, v);
			transpose_32x32(v);
#pragma unroll
			for(int c = 0; c < 32; ++c){ stage[c] = v[c]; }
		}
		else{
			uint32_t cur = OVERLAP_NO_COLUMN;
#pragma unroll 1
			for(uint32_t c = 0; c < OVERLAP_BLOCK; ++c){
				const uint32_t column = blk->column[c];
				uint32_t w = 0;
				if(column != OVERLAP_NO_COLUMN){
					if(column/32 != cur){
						cur = column/32;
						overlap_stage_rows(load, stride, cur, 0xFFFFFFFFu, first_row, end_row, v);
					}
					w = overlap_column_word(v, column%32);
				}
				stage[c] = w;
			}
		}
		__syncthreads();
		const uint32_t steps = (uint32_t)std::min<uint64_t>(OVERLAP_STEP_GROUPS, g_end - g0);
		for(uint32_t g = 0; g < steps; ++g){
			uint32_t wa[2], wb[2];
#pragma unroll
			for(int i = 0; i < 2; ++i){
				wa[i] = frag_a[i*OVERLAP_LDS_BLOCK + g*OVERLAP_LDS_PITCH];
				wb[i] = frag_b[i*OVERLAP_LDS_BLOCK + g*OVERLAP_LDS_PITCH];
			}
			overlap_v4i fa[2], fb[2];
#pragma unroll
			for(int i = 0; i < 2; ++i){
#pragma unroll
				for(int e = 0; e < 4; ++e){
					fa[i][e] = (int)overlap_spread(wa[i], h, (uint32_t)e);
					fb[i][e] = (int)overlap_spread(wb[i], h, (uint32_t)e);
				}
			}
#pragma unroll
			for(int i = 0; i < 2; ++i){
#pragma unroll
				for(int j = 0; j < 2; ++j){ acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0); }
			}
		}
		__syncthreads();
	}

	const bool mirror = p.symmetric && tl.ta != tl.tb;
	uint32_t *part_tile = p.partial ? p.partial + ((uint64_t)part*p.n_tiles + tile)*OVERLAP_TILE_CELLS : nullptr;
#pragma unroll
	for(int i = 0; i < 2; ++i){
#pragma unroll
		for(int j = 0; j < 2; ++j){
#pragma unroll
			for(int reg = 0; reg < 16; ++reg){
				const uint32_t row = (2*wm + i)*OVERLAP_BLOCK + (reg & 3) + 8*(reg >> 2) + 4*h;
				const uint32_t col = (2*wn + j)*OVERLAP_BLOCK + r;
				const uint32_t val = (uint32_t)acc[i][j][reg];
				if(part_tile){ part_tile[row*OVERLAP_TILE + col] = val; }
				else{ overlap_store_cell(p, mirror, (uint64_t)tl.ta*OVERLAP_TILE + row, (uint64_t)tl.tb*OVERLAP_TILE + col, val); }
			}
		}
	}
}

// overlap_combine_kernel: one lane per cell of every tile sums the cell's partial values of all parts and stores the
// cell (and its mirror) once.  Consecutive lanes consecutive columns of a tile row.
__global__ __launch_bounds__(OVERLAP_THREADS) void overlap_combine_kernel(OverlapArgs p)
{
	const uint64_t idx = (uint64_t)blockIdx.x*OVERLAP_THREADS + threadIdx.x;
	const uint32_t tile = (uint32_t)(idx/OVERLAP_TILE_CELLS), cell = (uint32_t)(idx%OVERLAP_TILE_CELLS);
	if(tile >= p.n_tiles){ return; }
	const OverlapTile tl = p.tiles[tile];
	uint32_t sum = 0;
	for(uint32_t part = 0; part < p.splits; ++part){ sum += p.partial[((uint64_t)part*p.n_tiles + tile)*OVERLAP_TILE_CELLS + cell]; }
	overlap_store_cell(p, p.symmetric && tl.ta != tl.tb, (uint64_t)tl.ta*OVERLAP_TILE + cell/OVERLAP_TILE, (uint64_t)tl.tb*OVERLAP_TILE + cell%OVERLAP_TILE, sum);
}

}  // namespace kwage

#endif
