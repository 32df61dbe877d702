// kwage_amd/csrc/topk_kernels.hpp -- gfx950 kernels of the top-k search (kwage_search_topk): for every query the k
// columns with the highest counts, selected on the device.  Included by topk.hip only, AFTER kernels.hpp: the tile
// decomposition, the counting loop, the real-column mask, the bit-sliced comparator and the segment sums are
// kernels.hpp's own (tile_coords, tile_lane, count_kmers, valid_mask, planes_ge, combine_segments, count_kernel's SEG form).
//
//   topk_tile_kernel     one wave = one query x 64 units of 16 B = 8192 columns: tile_lane, count_kmers, then a
//                        per-tile selection in place of emit_count_hits: the tile's best <= k columns go to the
//                        tile's own slot range of the candidate buffer (no atomic anywhere).
//   topk_combine_kernel  long queries: count_kernel<SEG> leaves partial counters per segment; combine_segments adds
//                        them up and wave 0 selects the same way.
//   topk_merge_kernel    one workgroup per query: radix select over the tiles' candidates, the <= k winners written
//                        ordered by column.
//   topk_append_kernel   kwage_search_topk_device_append: the selected records appended to the caller's device list.
//
// Candidates are 64-bit keys: score << 32 | (~column).  Keys of one query are distinct (columns are), and key order
// descending is exactly the contract's (score descending, column ascending).
#ifndef KWAGE_AMD_TOPK_KERNELS_HPP
#define KWAGE_AMD_TOPK_KERNELS_HPP

namespace kwage {

extern "C" __device__ uint32_t __ockl_wfred_add_u32(uint32_t);     // wave-wide sum (DPP), what __reduce_add_sync lowers to

struct TopkArgs {
	uint32_t k;
	uint32_t tiles;                 // tiles per query (8192 columns each)
	unsigned long long *cand;       // [query][tile][k] keys, the first cand_n[query][tile] of each range written
	uint32_t *cand_n;               // [query][tile]
};

__device__ __forceinline__ unsigned long long topk_key(uint32_t score, uint32_t column)
{
	return ((unsigned long long)score << 32) | (unsigned long long)(~column);
}

__device__ __forceinline__ uint32_t popc4(u32x4 m) { return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return __ockl_wfred_add_u32(v); }

// exclusive prefix sum over the 64 lanes
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	uint32_t incl = v;
#pragma unroll
	for(int d = 1; d < WAVE; d <<= 1){
		const uint32_t up = __shfl_up(incl, d);
		if(lane >= (uint32_t)d){ incl += up; }
	}
	return incl - v;
}

// The selection of one tile: the lane holds the bit-sliced counters of its 128 columns (unit*128 ...), `ok` marks the
// real ones (valid bits of a live lane).  Eligible: count >= f.  At most k eligible: all of them.  Otherwise the largest
// s with #(count >= s) >= k (binary search over [f, n], a wave-wide count per step), every column above s, and the
// columns AT s in ascending column order until k are taken.  Written in ascending column order to `out` (k slots);
// *out_n receives how many.  Every lane of the wave calls it.
template <int PLANES>
__device__ __forceinline__ void topk_select_tile(const u32x4 (&plane)[PLANES], u32x4 ok, uint32_t f, uint32_t n, uint32_t k,
                                                 uint32_t unit, unsigned long long *out, uint32_t *out_n)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	u32x4 sel = planes_ge<PLANES>(plane, f) & ok;
	uint32_t total = wave_sum(popc4(sel));
	if(total > k){
		uint32_t lo = f, hi = n;                // invariant: #(count >= lo) >= k
		while(lo < hi){
			const uint32_t mid = lo + (hi - lo + 1)/2;
			if(wave_sum(popc4(planes_ge<PLANES>(plane, mid) & ok)) >= k){ lo = mid; } else { hi = mid - 1; }
		}
		const u32x4 gt = (lo < n) ? (planes_ge<PLANES>(plane, lo + 1) & ok) : (u32x4)(0u);
		const u32x4 eq = planes_ge<PLANES>(plane, lo) & ok & ~gt;
		const uint32_t need = k - wave_sum(popc4(gt));      // > 0: #(count > lo) < k
		const uint32_t before = wave_excl_scan(popc4(eq));  // columns at lo in the lanes below
		uint32_t left = (before < need) ? need - before : 0u;
		sel = gt;
#pragma unroll
		for(int d = 0; d < 4; ++d){
			uint32_t bits = eq[d];
			if((uint32_t)__popc(bits) <= left){ sel[d] |= bits; left -= __popc(bits); continue; }
			while(left){ const uint32_t low = bits & (0u - bits); sel[d] |= low; bits ^= low; --left; }
		}
		total = k;
	}
	uint32_t at = wave_excl_scan(popc4(sel));
#pragma unroll
	for(int d = 0; d < 4; ++d){
		uint32_t bits = sel[d];
		while(bits){
			const uint32_t b = __ffs(bits) - 1;
			bits &= bits - 1;
			uint32_t cnt = 0;
#pragma unroll
			for(int p = 0; p < PLANES; ++p){ cnt |= ((plane[p][d] >> b) & 1u) << p; }
			out[at++] = topk_key(cnt, unit*128u + d*32u + b);
		}
	}
	if(lane == 0){ *out_n = total; }
}

template <int PLANES, int NH>
__global__ __launch_bounds__(SEARCH_THREADS) void topk_tile_kernel(SearchArgs a, TopkArgs t)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint64_t tile = (uint64_t)blockIdx.x*(SEARCH_THREADS/WAVE) + (threadIdx.x >> 6);
	if(tile >= (uint64_t)a.n_queries*a.chunks){ return; }
	uint32_t q, sg, c;
	tile_coords(a, tile, q, sg, c);         // (segs == 1)
	const uint64_t slot = (uint64_t)q*a.chunks + c;
	const uint32_t n = a.nkmer[q];
	if(n == 0){                             // kwage.cpp:369-371: no k-mers, no hits
		if(lane == 0){ t.cand_n[slot] = 0; }
		return;
	}
	const uint32_t *rq = a.rows + a.pos_off[q]*NH;
	uint32_t u0, unit;
	bool live;
	tile_lane(a, c, lane, u0, live, unit);
	u32x4 plane[PLANES];
#pragma unroll
	for(int p = 0; p < PLANES; ++p){ plane[p] = (u32x4)(0u); }
	(void)count_kmers<PLANES, NH>(a.db, a.stride, rq, n, unit, plane, [](uint32_t) -> bool { return false; });
	const u32x4 ok = valid_mask(a, unit, live);
	topk_select_tile<PLANES>(plane, ok, a.qthr[q], n, t.k, unit, t.cand + slot*t.k, t.cand_n + slot);
}

// combine_segments over the segments' partial counters, then the tile selection by wave 0.  One workgroup per (query, tile of 64 units).
template <int PLANES>
__global__ __launch_bounds__(COMBINE_WAVES*WAVE) void topk_combine_kernel(SearchArgs a, TopkArgs t, uint32_t seg_planes)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char topk_combine_lds[];     // (COMBINE_WAVES/2) x PLANES x 64 x 16 B
	u32x4 (*red)[PLANES][WAVE] = reinterpret_cast<u32x4 (*)[PLANES][WAVE]>(topk_combine_lds);
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t q = blockIdx.x / a.chunks, c = blockIdx.x % a.chunks;
	const uint64_t slot = (uint64_t)q*a.chunks + c;
	const uint32_t n = a.nkmer[q];
	if(n == 0){                                            // uniform per workgroup
		if(threadIdx.x == 0){ t.cand_n[slot] = 0; }
		return;
	}
	uint32_t u0, unit;
	bool on;
	tile_lane(a, c, lane, u0, on, unit);
	u32x4 plane[PLANES];
#pragma unroll
	for(int p = 0; p < PLANES; ++p){ plane[p] = (u32x4)(0u); }
	combine_segments<PLANES>(a, q, unit, n, seg_planes, w, lane, red, plane);
	if(w == 0){
		const u32x4 ok = valid_mask(a, unit, on);
		topk_select_tile<PLANES>(plane, ok, a.qthr[q], n, t.k, unit, t.cand + slot*t.k, t.cand_n + slot);
	}
}

static constexpr int MERGE_THREADS = 256;

// One workgroup per query: the <= k largest keys among the query's tiles x k candidate slots (slot j of the flat range
// is a candidate when j % k < cand_n[j / k]).  Radix select, 8 bits at a time from the top, finds the k-th largest key
// T; then every candidate >= T is written, in slot order -- tile by tile, ascending columns within a tile: ascending
// columns -- to out[q*k ...], the count to out_n[q].  `q_base` is added to the query index of the records.
__global__ __launch_bounds__(MERGE_THREADS) void topk_merge_kernel(TopkArgs t, uint32_t q_base, kwage_hit *out, uint32_t *out_n)
{
	__shared__ uint32_t hist[256];
	__shared__ uint32_t wave_tot[MERGE_THREADS/WAVE];
	__shared__ unsigned long long s_prefix;
	__shared__ uint32_t s_want;
	const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6;
	const uint32_t k = t.k;
	const uint64_t slots = (uint64_t)t.tiles*k;
	const unsigned long long *cq = t.cand + (uint64_t)q*slots;
	const uint32_t *nq = t.cand_n + (uint64_t)q*t.tiles;
	auto is_cand = [&](uint64_t j) -> bool { return (uint32_t)(j % k) < nq[j / k]; };

	// total candidates
	uint32_t mine = 0;
	for(uint32_t i = tid; i < t.tiles; i += MERGE_THREADS){ mine += nq[i]; }
	mine = wave_sum(mine);
	if(lane == 0){ wave_tot[w] = mine; }
	__syncthreads();
	uint32_t total = 0;
	for(int i = 0; i < MERGE_THREADS/WAVE; ++i){ total += wave_tot[i]; }
	__syncthreads();

	unsigned long long thr = 0;             // keys >= thr are selected (all of them when there are at most k)
	if(total > k){
		unsigned long long prefix = 0, mask = 0;
		uint32_t want = k;                  // rank, from the top, of the k-th largest key among those matching prefix
		for(int shift = 56; shift >= 0; shift -= 8){
			hist[tid] = 0;
			__syncthreads();
			for(uint64_t j = tid; j < slots; j += MERGE_THREADS){
				if(!is_cand(j)){ continue; }
				const unsigned long long key = cq[j];
				if((key & mask) == prefix){ atomicAdd(&hist[(key >> shift) & 255u], 1u); }
			}
			__syncthreads();
			if(tid == 0){
				uint32_t above = 0;
				int b = 255;
				for(; b > 0 && above + hist[b] < want; --b){ above += hist[b]; }
				s_want = want - above;
				s_prefix = prefix | ((unsigned long long)b << shift);
			}
			__syncthreads();
			want = s_want;
			prefix = s_prefix;
			mask |= 255ull << shift;
			__syncthreads();
		}
		thr = prefix;                       // keys are distinct: exactly k keys are >= the k-th largest
	}

	// ordered compaction, MERGE_THREADS slots at a time
	kwage_hit *oq = out + (uint64_t)q*k;
	uint32_t base = 0;
	for(uint64_t j0 = 0; j0 < slots; j0 += MERGE_THREADS){
		const uint64_t j = j0 + tid;
		unsigned long long key = 0;
		bool take = false;
		if(j < slots && is_cand(j)){ key = cq[j]; take = key >= thr; }
		const unsigned long long ball = __ballot(take);
		const uint32_t rank = __popcll(ball & ((1ull << lane) - 1ull));
		if(lane == 0){ wave_tot[w] = __popcll(ball); }
		__syncthreads();
		uint32_t off = base;
		for(uint32_t i = 0; i < w; ++i){ off += wave_tot[i]; }
		uint32_t step = 0;
		for(int i = 0; i < MERGE_THREADS/WAVE; ++i){ step += wave_tot[i]; }
		if(take){
			const uint32_t at = off + rank;
			if(at < k){
				kwage_hit h;
				h.query = q_base + q;
				h.column = ~(uint32_t)key;
				h.num_match = (uint32_t)(key >> 32);
				oq[at] = h;
			}
		}
		base += step;
		__syncthreads();
	}
	if(tid == 0){ out_n[q] = min(base, k); }
}

// kwage_search_topk_device_append's output stage: query q's <= k selected records (sel[q*k ...], ordered by column) go
// to out[base + off[q] ...] with column_base added to the column; records at or beyond `capacity` are not written (the
// host has counted them).  One workgroup per query.
__global__ __launch_bounds__(WAVE) void topk_append_kernel(const kwage_hit *sel, const uint32_t *sel_n, uint32_t k,
                                                          const unsigned long long *off, unsigned long long base,
                                                          uint32_t column_base, kwage_hit *out, unsigned long long capacity)
{
	const uint32_t q = blockIdx.x;
	const uint32_t m = min(sel_n[q], k);
	const unsigned long long o = base + off[q];
	for(uint32_t i = threadIdx.x; i < m; i += WAVE){
		if(o + i >= capacity){ break; }
		kwage_hit h = sel[(uint64_t)q*k + i];
		h.column += column_base;
		out[o + i] = h;
	}
}

}  // namespace kwage

#endif
