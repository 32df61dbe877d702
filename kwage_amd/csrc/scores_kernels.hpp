// kwage_amd/csrc/scores_kernels.hpp -- gfx950 kernels of the dense score search (kwage_search_scores): every query's
// k-mer count for every column of a group, written as a queries x columns matrix of uint32 cells.  Included by
// scores.hip only, AFTER kernels.hpp: the tile decomposition, the counting loop, the real-column mask and the segment
// sums are kernels.hpp's own (tile_coords, tile_lane, count_kmers, valid_mask, combine_segments, count_kernel's SEG form).
//
//   score_tile_kernel     one wave = one query x 64 units of 16 B = 8192 columns: tile_lane, count_kmers, then the
//                         expand-and-store epilogue in place of emit_count_hits: no atomic, no hit list.
//   score_combine_kernel  long queries: count_kernel<SEG> leaves partial counters per segment; combine_segments adds
//                         them up and wave 0 runs the same epilogue.
//
// The epilogue turns the bit-sliced counters of a tile -- PLANES x 4 dwords per lane for the lane's 128 consecutive
// columns -- into 8192 cells (32 KiB) in 16-byte stores.  Two forms, chosen per launch (ScoreArgs::form):
//   SCORES_FORM_WAVE  every store instruction writes 1 KiB of consecutive cells (64 lanes x 16 B): the planes of two
//                     lanes at a time are what the 64 lanes expand, so the planes cross lanes through the wave's own
//                     piece of LDS, 8 or 16 lanes' worth at a time (at most 4 KiB per wave).
//   SCORES_FORM_LANE  every lane expands its own 128 columns and stores its own 512-byte run: nothing crosses lanes,
//                     a store instruction touches 64 separate cache lines.
#ifndef KWAGE_AMD_SCORES_KERNELS_HPP
#define KWAGE_AMD_SCORES_KERNELS_HPP

#include "score_stage.hpp"      // ScoreArgs, SCORES_FORM_*

namespace kwage {

// lanes whose planes lie in LDS at a time in the wave form: PLANES x lanes x 16 B <= 4 KiB per wave
template <int PLANES> struct ScoreXch { static constexpr int LANES = (PLANES <= 14) ? 16 : 8; };

// Four cells from one dword of every plane: bits sh .. sh+3 of x[p] are bit p of the cells 0 .. 3.  A nibble times
// 0x00204081 has its bit j at bit 8j: eight planes at a time collect in the bytes of one dword.
template <int PLANES, typename LOADX>
__device__ __forceinline__ u32x4 expand4(uint32_t sh, LOADX loadx)
{
	constexpr int G = (PLANES + 7)/8;
	uint32_t acc[G];
#pragma unroll
	for(int g = 0; g < G; ++g){ acc[g] = 0; }
#pragma unroll
	for(int p = 0; p < PLANES; ++p){
		const uint32_t spread = __umul24((loadx(p) >> sh) & 15u, 0x00204081u) & 0x01010101u;
		acc[p >> 3] |= spread << (p & 7);
	}
	u32x4 cell;
#pragma unroll
	for(int j = 0; j < 4; ++j){
		uint32_t v = 0;
#pragma unroll
		for(int g = 0; g < G; ++g){ v |= ((acc[g] >> (8*j)) & 255u) << (8*g); }
		cell[j] = v;
	}
	return cell;
}

// The epilogue of one tile; every lane of the wave calls it.  `plane`: the lane's counters, pad columns and dead lanes
// already zero.  `row`: the query's row of the matrix, col0: the tile's first column.  `xch`: the wave's own
// PLANES x ScoreXch<PLANES>::LANES x 16 B of LDS (wave form only).
template <int PLANES>
__device__ __forceinline__ void store_scores(const ScoreArgs &sa, const u32x4 (&plane)[PLANES], uint32_t *row, unsigned long long col0, u32x4 *xch)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	if(sa.form == SCORES_FORM_LANE){
#pragma unroll
		for(int d = 0; d < 4; ++d){
#pragma unroll 1
			for(uint32_t nib = 0; nib < 8; ++nib){
				const u32x4 cell = expand4<PLANES>(nib*4u, [&](int p) -> uint32_t { return plane[p][d]; });
				const unsigned long long col = col0 + lane*128u + d*32u + nib*4u;
				if(col < sa.span){ *reinterpret_cast<u32x4*>(row + col) = cell; }
			}
		}
		return;
	}
	constexpr int LR = ScoreXch<PLANES>::LANES;
	const uint32_t *x32 = reinterpret_cast<const uint32_t*>(xch);
	// lanes 0-31 expand the round's lane 2j, lanes 32-63 lane 2j + 1: dword (lane / 8) % 4, nibble lane % 8
	const uint32_t half = lane >> 5, d = (lane >> 3) & 3u, sh = (lane & 7u)*4u;
#pragma unroll 1
	for(uint32_t r = 0; r < (uint32_t)(WAVE/LR); ++r){
		if(lane/LR == r){
#pragma unroll
			for(int p = 0; p < PLANES; ++p){ xch[p*LR + (lane % LR)] = plane[p]; }
		}
		// Writers and readers are lanes of ONE wave, and xch is that wave's own: the LDS operations of a wave complete in
		// the order it issues them, so the reads below see the writes above with no wait between them -- the fences only
		// keep the compiler from reordering.  Lanes of another wave would need a workgroup fence and barrier here.
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
		for(uint32_t j = 0; j < (uint32_t)(LR/2); ++j){
			const uint32_t src = 2u*j + half;
			const u32x4 cell = expand4<PLANES>(sh, [&](int p) -> uint32_t { return x32[(p*LR + src)*4u + d]; });
			const unsigned long long col = col0 + (r*(LR/2) + j)*256u + lane*4u;
			if(col < sa.span){ *reinterpret_cast<u32x4*>(row + col) = cell; }
		}
		// (the same in the other direction: the round's reads are done before the next round's writes)
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
	}
}

template <int PLANES, int NH>
__global__ __launch_bounds__(SEARCH_THREADS) void score_tile_kernel(SearchArgs a, ScoreArgs sa)
{
	__shared__ u32x4 xch[SEARCH_THREADS/WAVE][PLANES*ScoreXch<PLANES>::LANES];
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint64_t tile = (uint64_t)blockIdx.x*(SEARCH_THREADS/WAVE) + (threadIdx.x >> 6);
	if(tile >= (uint64_t)a.n_queries*a.chunks){ return; }
	uint32_t q, sg, c;
	tile_coords(a, tile, q, sg, c);         // (segs == 1)
	const uint32_t n = a.nkmer[q];
	uint32_t u0, unit;
	bool live;
	tile_lane(a, c, lane, u0, live, unit);
	u32x4 plane[PLANES];
#pragma unroll
	for(int p = 0; p < PLANES; ++p){ plane[p] = (u32x4)(0u); }
	if(n){                                  // (a query without k-mers: a row of zeros)
		const uint32_t *rq = a.rows + a.pos_off[q]*NH;
		(void)count_kmers<PLANES, NH>(a.db, a.stride, rq, n, unit, plane, [](uint32_t) -> bool { return false; });
		const u32x4 ok = valid_mask(a, unit, live);
#pragma unroll
		for(int p = 0; p < PLANES; ++p){ plane[p] &= ok; }
	}
	store_scores<PLANES>(sa, plane, sa.out + (unsigned long long)q*sa.row_elems, (unsigned long long)c*(WAVE*128u), xch[threadIdx.x >> 6]);
}

// combine_segments over the segments' partial counters, then the epilogue by wave 0, which takes the tree's LDS for its
// exchange.  One workgroup per (query, tile of 64 units).
template <int PLANES>
__global__ __launch_bounds__(COMBINE_WAVES*WAVE) void score_combine_kernel(SearchArgs a, ScoreArgs sa, uint32_t seg_planes)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char score_combine_lds[];     // (COMBINE_WAVES/2) x PLANES x 64 x 16 B
	u32x4 (*red)[PLANES][WAVE] = reinterpret_cast<u32x4 (*)[PLANES][WAVE]>(score_combine_lds);
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t q = blockIdx.x / a.chunks, c = blockIdx.x % a.chunks;
	const uint32_t n = a.nkmer[q];
	uint32_t u0, unit;
	bool on;
	tile_lane(a, c, lane, u0, on, unit);
	u32x4 plane[PLANES];
#pragma unroll
	for(int p = 0; p < PLANES; ++p){ plane[p] = (u32x4)(0u); }
	if(n){                                                 // uniform per workgroup
		combine_segments<PLANES>(a, q, unit, n, seg_planes, w, lane, red, plane);
	}
	if(w == 0){
		const u32x4 ok = valid_mask(a, unit, on);
#pragma unroll
		for(int p = 0; p < PLANES; ++p){ plane[p] &= ok; }
		store_scores<PLANES>(sa, plane, sa.out + (unsigned long long)q*sa.row_elems, (unsigned long long)c*(WAVE*128u),
		                     reinterpret_cast<u32x4*>(score_combine_lds));
	}
}

}  // namespace kwage

#endif
