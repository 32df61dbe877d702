// kwage_amd/csrc/presence_kernels.hpp -- gfx950 kernels of the presence search (kwage_search_presence): one bit per
// (query, column), set where the column's k-mer count reaches the query's floor, in the byte order of a row of the
// matrix.  Included by presence.hip only, AFTER kernels.hpp: the tile decomposition, the counting loop, the early-exit
// rule, the comparator and the segment sums are kernels.hpp's own (tile_coords, tile_lane, count_kmers,
// tile_cannot_pass, planes_ge, combine_segments, count_kernel's SEG form).
//
//   presence_tile_kernel     one wave = one query x 64 units of 16 B = 8192 columns: tile_lane, count_kmers with
//                            tile_cannot_pass as its stop rule, then planes_ge & valid stored as ONE 16-byte store per
//                            lane: the lane's four dwords already are the matrix's bytes for its 128 columns.  No LDS,
//                            no cross-lane traffic, no atomic.
//   presence_combine_kernel  long queries: count_kernel<SEG> leaves partial counters per segment; combine_segments adds
//                            them up and wave 0 compares and stores.
//   presence_and_kernel      floor == the k-mer count (t = 1): and_kernel's loop, the accumulator & valid stored.
//   presence_popcount_kernel the set bits of every query's row (asked for only with `passing`).
//
// Every (query, tile) stores its 16-byte units below w_units whatever it found -- a tile given up by the early exit and
// a query without k-mers store zeros -- so the bitmap never has to be cleared beforehand.
#ifndef KWAGE_AMD_PRESENCE_KERNELS_HPP
#define KWAGE_AMD_PRESENCE_KERNELS_HPP

namespace kwage {

struct PresenceArgs {
	uint8_t *out;                   // bit (q, c) of the launch's queries at out[q*row_bytes + c/8], bit c%8
	unsigned long long row_bytes;   // bytes between rows (multiple of 16)
	uint32_t w_units;               // 16-byte units written per row: the group's row bytes rounded up to 16 (<= units_per_row)
	int early_exit;                 // KWAGE_SEARCH_EARLY_EXIT: a tile in which no column can pass any more stops
};

static constexpr int POPCOUNT_THREADS = 256;

// the lane's 16 bytes of the row of query q; lanes at or beyond the row's end store nothing
__device__ __forceinline__ void store_presence(const PresenceArgs &pa, uint32_t q, uint32_t u0, u32x4 bits)
{
	if(u0 < pa.w_units){ *reinterpret_cast<u32x4*>(pa.out + (unsigned long long)q*pa.row_bytes + (unsigned long long)u0*16u) = bits; }
}

template <int PLANES, int NH>
__global__ __launch_bounds__(SEARCH_THREADS) void presence_tile_kernel(SearchArgs a, PresenceArgs pa)
{
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint64_t tile = (uint64_t)blockIdx.x*(SEARCH_THREADS/WAVE) + (threadIdx.x >> 6);
	if(tile >= (uint64_t)a.n_queries*a.chunks){ return; }
	uint32_t q, sg, c;
	tile_coords(a, tile, q, sg, c);         // (segs == 1)
	const uint32_t n = a.nkmer[q];
	uint32_t u0, unit;
	bool live;
	tile_lane(a, c, lane, u0, live, unit);
	u32x4 bits = (u32x4)(0u);
	if(n){                                  // (a query without k-mers: a row of zeros)
		const uint32_t thr = a.qthr[q];
		const uint32_t *rq = a.rows + a.pos_off[q]*NH;
		u32x4 plane[PLANES];
	#pragma unroll
	for(int p = 0; p < PLANES; ++p){ plane[p] = (u32x4)(0u); }
		const bool whole = count_kmers<PLANES, NH>(a.db, a.stride, rq, n, unit, plane, [&](uint32_t done) -> bool {
			return pa.early_exit && tile_cannot_pass<PLANES>(plane, thr, n - done);
		});
		if(whole && live){ bits = planes_ge<PLANES>(plane, thr) & reinterpret_cast<const u32x4*>(a.valid)[unit]; }
	}
	store_presence(pa, q, u0, bits);
}

// combine_segments over the segments' partial counters, then the compare-and-store by wave 0.  One workgroup per
// (query, tile of 64 units).
template <int PLANES>
__global__ __launch_bounds__(COMBINE_WAVES*WAVE) void presence_combine_kernel(SearchArgs a, PresenceArgs pa, uint32_t seg_planes)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char presence_combine_lds[];     // (COMBINE_WAVES/2) x PLANES x 64 x 16 B
	u32x4 (*red)[PLANES][WAVE] = reinterpret_cast<u32x4 (*)[PLANES][WAVE]>(presence_combine_lds);
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
		u32x4 bits = (u32x4)(0u);
		if(n && on){ bits = planes_ge<PLANES>(plane, a.qthr[q]) & reinterpret_cast<const u32x4*>(a.valid)[unit]; }
		store_presence(pa, q, u0, bits);
	}
}

// The floor is the k-mer count: a column passes iff it is set in every addressed row (and_kernel<1, false>'s loop over
// the KiB tile: eight rows in flight, nontemporal loads).  With the early exit a tile stops after any group of eight
// rows that leaves no bit in the wave: its accumulators are all zero then, which is what it stores.
__global__ __launch_bounds__(SEARCH_THREADS) void presence_and_kernel(SearchArgs a, PresenceArgs pa)
{
	constexpr int UNROLL = 8;
	const uint32_t lane = threadIdx.x & (WAVE - 1);
	const uint64_t tile = (uint64_t)blockIdx.x*(SEARCH_THREADS/WAVE) + (threadIdx.x >> 6);
	if(tile >= (uint64_t)a.n_queries*a.chunks){ return; }
	uint32_t q, sg, c;
	tile_coords(a, tile, q, sg, c);         // (segs == 1)
	const uint32_t n = a.nkmer[q];
	uint32_t u0, unit;
	bool live;
	tile_lane(a, c, lane, u0, live, unit);
	u32x4 acc = (u32x4)(0u);
	if(n){
		const uint32_t nrows = n*a.num_hash;
		const uint32_t *rq = a.rows + a.pos_off[q]*a.num_hash;
		acc = ~(u32x4)(0u);
		uint32_t i = 0;
		bool dead = false;
		for(; i + UNROLL <= nrows; i += UNROLL){
			u32x4 x[UNROLL];
#pragma unroll
			for(int u = 0; u < UNROLL; ++u){
				const uint32_t r = rq[i + u];
				x[u] = load16<true>(reinterpret_cast<const u32x4*>(a.db + (uint64_t)r*a.stride) + unit);
			}
#pragma unroll
			for(int u = 0; u < UNROLL; ++u){ acc &= x[u]; }
			if(pa.early_exit && !__any((acc.x | acc.y | acc.z | acc.w) != 0)){ dead = true; break; }
		}
		for(; !dead && i < nrows; ++i){
			const uint32_t r = rq[i];
			acc &= load16<true>(reinterpret_cast<const u32x4*>(a.db + (uint64_t)r*a.stride) + unit);
		}
		acc = live ? (acc & reinterpret_cast<const u32x4*>(a.valid)[unit]) : (u32x4)(0u);
	}
	store_presence(pa, q, u0, acc);
}

// passing[q] = set bits of row q: one workgroup per query over the row's 16-byte units, summed through LDS.
__global__ __launch_bounds__(POPCOUNT_THREADS) void presence_popcount_kernel(PresenceArgs pa, uint32_t *passing)
{
	__shared__ uint32_t part[POPCOUNT_THREADS];
	const uint32_t q = blockIdx.x;
	const u32x4 *row = reinterpret_cast<const u32x4*>(pa.out + (unsigned long long)q*pa.row_bytes);
	uint32_t cnt = 0;
	for(uint32_t u = threadIdx.x; u < pa.w_units; u += POPCOUNT_THREADS){
		const u32x4 v = row[u];
		cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
	}
	part[threadIdx.x] = cnt;
	__syncthreads();
#pragma unroll
	for(int half = POPCOUNT_THREADS/2; half >= 1; half >>= 1){
		if(threadIdx.x < (uint32_t)half){ part[threadIdx.x] += part[threadIdx.x + half]; }
		__syncthreads();
	}
	if(threadIdx.x == 0){ passing[q] = part[0]; }
}

}  // namespace kwage

#endif
