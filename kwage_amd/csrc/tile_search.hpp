// kwage_amd/csrc/tile_search.hpp -- the launches of a counted tile search: for every query of a row-list view a tile
// kernel per KiB tile of the group's rows, or (long queries) count_kernel's SEG form over the segments and a combine
// kernel per tile, slice by slice of the queries as engine.hip's plan_tiles cut them.  Shared by topk.hip and scores.hip,
// which include it after kernels.hpp and name their kernels in a struct K:
//
//   K::Epi                               the argument of the kernels' epilogue (TopkArgs, ScoreArgs)
//   K::tile<PLANES, NH>()                the tile kernel:     __global__ void(SearchArgs, Epi)
//   K::combine<PLANES>()                 the combine kernel:  __global__ void(SearchArgs, Epi, uint32_t seg_planes)
//   K::tile_name, K::seg_name            printf formats of the reported kernel name: (planes, nh), (seg_planes, nh, planes)
//
// Everything here is a template or inline: a unit that does not call it instantiates nothing.
#ifndef KWAGE_AMD_TILE_SEARCH_HPP
#define KWAGE_AMD_TILE_SEARCH_HPP

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "engine_state.hpp"
#include "pool_blocks.hpp"

namespace kwage {

// (by_planes, by_shape: the dispatch on counter width and hash count, engine_state.hpp)

// partial counters of every (query, segment, tile) of the launch into a.partial
inline void launch_seg_count(const SearchArgs &a, uint32_t seg_planes, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a.n_queries*a.segs*a.chunks;
	by_shape(seg_planes, a.num_hash, [&](auto P, auto NH) {
		hipLaunchKernelGGL((count_kernel<decltype(P)::value, decltype(NH)::value, true>), dim3((uint32_t)((tiles + 3)/4)),
		                   dim3(SEARCH_THREADS), 0, s, a);
	});
}

// the segments' sum and the search's epilogue: one workgroup per (query, tile), the tree's LDS sized by the planes
template <typename K>
int launch_combine(uint32_t planes, const SearchArgs &a, const typename K::Epi &e, uint32_t seg_planes, hipStream_t s)
{
	return by_planes(planes, [&](auto P) -> int {
		constexpr int PLANES = decltype(P)::value;
		constexpr size_t lds = (size_t)(COMBINE_WAVES/2)*PLANES*WAVE*16;
		const auto kernel = K::template combine<PLANES>();
		int rc;
		if((rc = allow_dynamic_lds(kernel, lds))){ return rc; }
		hipLaunchKernelGGL(kernel, dim3(a.n_queries*a.chunks), dim3(COMBINE_WAVES*WAVE), lds, s, a, e, seg_planes);
		return KWAGE_OK;
	});
}

// The search over the lists of `v` in group g, queued on s: the tile form, or segments + combine, for one slice of the
// plan after the other; after_slice(a, q0) follows each (a: the slice's launch arguments, q0: its first list) and may
// change what `e` refers to for the next.  qthr: the lists' floors (null: none).  kernel_name receives 64 bytes.
template <typename K, typename After>
int run_tile_slices(const kwage_group *g, const RowListView &v, const uint32_t *qthr, const TilePlan &plan, const typename K::Epi &e,
                    PoolBlocks &blocks, char *kernel_name, hipStream_t s, After &&after_slice)
{
	int rc;
	SearchArgs a;
	memset(&a, 0, sizeof(a));
	a.db = g->d_bits;
	a.stride = g->stride;
	a.units_per_row = plan.units_per_row;
	a.valid = g->d_valid;
	a.rows = v.rows;
	a.num_hash = v.num_hash;
	a.chunks = plan.chunks;
	a.segs = plan.segs;
	a.seg_kmers = plan.seg_kmers;
	if(a.segs > 1){
		uint32_t *slab = nullptr;
		if((rc = blocks.take((uint64_t)plan.slice*a.segs*plan.seg_planes*g->stride, &slab))){ return rc; }
		a.partial = slab;
		snprintf(kernel_name, 64, K::seg_name, plan.seg_planes, std::min(v.num_hash, 5u), plan.planes);
	}
	else{
		snprintf(kernel_name, 64, K::tile_name, plan.planes, std::min(v.num_hash, 5u));
	}
	for(uint32_t q0 = 0; q0 < v.n; q0 += plan.slice){
		a.n_queries = std::min(plan.slice, v.n - q0);
		a.pos_off = v.pos_off + q0;
		a.nkmer = v.counts + q0;
		a.qthr = qthr ? qthr + q0 : nullptr;
		if(a.segs > 1){
			launch_seg_count(a, plan.seg_planes, s);
			HIP_TRY(hipGetLastError());
			if((rc = launch_combine<K>(plan.planes, a, e, plan.seg_planes, s))){ return rc; }
		}
		else{
			const uint64_t tiles = (uint64_t)a.n_queries*a.chunks;
			by_shape(plan.planes, v.num_hash, [&](auto P, auto NH) {
				hipLaunchKernelGGL((K::template tile<decltype(P)::value, decltype(NH)::value>()), dim3((uint32_t)((tiles + 3)/4)),
				                   dim3(SEARCH_THREADS), 0, s, a, e);
			});
		}
		HIP_TRY(hipGetLastError());
		if((rc = after_slice(a, q0))){ return rc; }
	}
	return KWAGE_OK;
}

}  // namespace kwage

#endif
