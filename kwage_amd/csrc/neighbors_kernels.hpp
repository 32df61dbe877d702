// kwage_amd/csrc/neighbors_kernels.hpp -- the kernels of the nearest-neighbour lists (neighbors.hip,
// kwage_group_column_neighbors) besides the overlap's: the set bits of every column of a resident matrix, and the
// selection of each entry's k best candidates from a strip of overlap cells.
//
//   neighbors_bits_kernel       a wave per (64 dwords of the row, part of the rows): every lane counts the 32 columns of
//                               its dword over the rows of its part into registers and stores the 32 partial counts
//   neighbors_bits_sum_kernel   a lane per column sums the parts' counts
//   neighbors_select_kernel     a workgroup per entry of the strip (the grid loops): exact 8-bit radix select, most
//                               significant byte first, of the k-th best (key, index) with histograms in LDS; the
//                               winners collected in LDS, ordered by a bitonic sort, stored with filler and count
//
// No global atomics, no floating point, nothing cleared beforehand: every output word is stored once.
#ifndef KWAGE_AMD_NEIGHBORS_KERNELS_HPP
#define KWAGE_AMD_NEIGHBORS_KERNELS_HPP

#include <hip/hip_runtime.h>

#include "neighbors_plan.hpp"

namespace kwage {

constexpr int NEIGHBORS_THREADS = 256;
constexpr int NEIGHBORS_BITS_THREADS = 64;
constexpr uint32_t NEIGHBORS_BITS_MAX_PARTS = 1024;

// Part p of `parts` takes the rows [rows p / parts, rows (p + 1) / parts); partial is [parts][32 dwords] counts.
__global__ __launch_bounds__(NEIGHBORS_BITS_THREADS) void neighbors_bits_kernel(const uint8_t *bits, unsigned long long stride, unsigned long long rows,
                                                                                 uint32_t dwords, uint32_t parts, uint32_t *partial)
{
	const uint32_t slabs = (dwords + NEIGHBORS_BITS_THREADS - 1)/NEIGHBORS_BITS_THREADS;
	const uint32_t slab = blockIdx.x % slabs, part = blockIdx.x / slabs;
	const uint32_t d = slab*NEIGHBORS_BITS_THREADS + threadIdx.x;
	if(d >= dwords || part >= parts){ return; }
	const uint64_t r0 = (uint64_t)rows*part/parts, r1 = (uint64_t)rows*(part + 1)/parts;
	uint32_t cnt[32];
#pragma unroll
	for(int b = 0; b < 32; ++b){ cnt[b] = 0; }
	const uint8_t *p = bits + 4ull*d;
	for(uint64_t r = r0; r < r1; ++r){
		const uint32_t w = *reinterpret_cast<const uint32_t*>(p + r*stride);
#pragma unroll
		for(int b = 0; b < 32; ++b){ cnt[b] += (w >> b) & 1u; }
	}
	uint4 *out = reinterpret_cast<uint4*>(partial + ((uint64_t)part*dwords + d)*32);
#pragma unroll
	for(int q = 0; q < 8; ++q){ out[q] = make_uint4(cnt[4*q], cnt[4*q + 1], cnt[4*q + 2], cnt[4*q + 3]); }
}

__global__ __launch_bounds__(NEIGHBORS_THREADS) void neighbors_bits_sum_kernel(const uint32_t *partial, uint32_t parts, uint32_t columns, uint32_t *out)
{
	const uint32_t c = blockIdx.x*NEIGHBORS_THREADS + threadIdx.x;
	if(c >= columns){ return; }
	uint32_t sum = 0;
	for(uint32_t p = 0; p < parts; ++p){ sum += partial[(uint64_t)p*columns + c]; }
	out[c] = sum;
}

struct NeighborsArgs {
	const uint32_t *cells;                 // the strip's block: [entries][pitch]
	unsigned long long pitch, n_b;
	unsigned long long entries, first_entry;   // of the strip; its first entry in a's list
	const uint32_t *col_a, *col_b;         // the column every entry of a's list / every candidate names, OVERLAP_NO_COLUMN for a dead one
	const uint32_t *bits_a, *bits_b;       // set bits by column of a's / b's group
	uint32_t k, metric, min_shared, skip_same, tie_bytes;
	kwage_neighbor *out;                   // [n_a][k]
	uint32_t *counts;                      // [n_a]
};

struct NeighborsLds {
	uint32_t hist[256];
	unsigned long long wkey[KWAGE_TOPK_MAX];
	uint32_t windex[KWAGE_TOPK_MAX];
	unsigned long long pkey;
	uint32_t ptie, want, eligible, done, n;
};

// Every eligible candidate of the entry whose row of cells is `row`: f(index, key).  A lane reads four cells with one
// 16-byte load (rows start at 16-byte boundaries of the block and are a multiple of four cells long; the cells between
// n_b and the pitch are read and not looked at).
template <typename F>
__device__ __forceinline__ void neighbors_visit(const NeighborsArgs &a, const uint32_t *row, uint32_t col_a, uint32_t bits_a, F &&f)
{
	if(col_a == OVERLAP_NO_COLUMN){ return; }         // (uniform per workgroup)
	for(uint64_t j0 = 4ull*threadIdx.x; j0 < a.n_b; j0 += 4ull*NEIGHBORS_THREADS){
		const uint4 c = *reinterpret_cast<const uint4*>(row + j0);
		const uint32_t s[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
		for(int t = 0; t < 4; ++t){
			const uint64_t j = j0 + t;
			if(j < a.n_b){
				const uint32_t cb = a.col_b[j];
				if(neighbors_eligible(col_a, cb, s[t], a.min_shared, a.skip_same != 0)){
					f((uint32_t)j, neighbors_key(a.metric, s[t], bits_a, a.bits_b[cb]));
				}
			}
		}
	}
}

__global__ __launch_bounds__(NEIGHBORS_THREADS) void neighbors_select_kernel(NeighborsArgs a)
{
	__shared__ NeighborsLds l;
	const uint32_t tid = threadIdx.x;
	for(uint64_t e = blockIdx.x; e < a.entries; e += gridDim.x){
		const uint64_t i = a.first_entry + e;
		const uint32_t col_a = a.col_a[i];
		const uint32_t bits_a = col_a != OVERLAP_NO_COLUMN ? a.bits_a[col_a] : 0u;
		const uint32_t *row = a.cells + neighbors_cell_offset(e, a.pitch, 0);

		// the cut: the k-th best composite, byte by byte from the top
		uint64_t pkey = 0;
		uint32_t ptie = 0;
		bool first = true;
		if(tid == 0){ l.want = a.k; l.done = 0; l.eligible = 0; l.pkey = 0; l.ptie = 0; }
		for(int byte = (int)(a.metric == KWAGE_NEIGHBORS_SHARED ? NEIGHBORS_KEY_TOP_SHARED : NEIGHBORS_KEY_TOP_JACCARD); byte >= 0; byte = neighbors_next_byte(byte, a.tie_bytes)){
			for(uint32_t h = tid; h < 256; h += NEIGHBORS_THREADS){ l.hist[h] = 0; }
			__syncthreads();
			neighbors_visit(a, row, col_a, bits_a, [&](uint32_t j, unsigned long long key) {
				const uint32_t tie = neighbors_tie(a.tie_bytes, j);
				if(neighbors_prefix_match(key, tie, pkey, ptie, byte)){ atomicAdd(&l.hist[neighbors_digit(key, tie, byte)], 1u); }
			});
			__syncthreads();
			if(tid == 0){
				bool done = false;
				if(first){
					uint32_t m = 0;
					for(int h = 0; h < 256; ++h){ m += l.hist[h]; }
					l.eligible = m;
					done = m <= a.k;                      // every eligible candidate wins: the cut stays at zero
				}
				if(!done){
					uint32_t want = l.want;
					uint64_t pk = l.pkey;
					uint32_t pt = l.ptie;
					const uint32_t d = neighbors_pick_digit(l.hist, want);
					neighbors_prefix_set(pk, pt, byte, d);
					l.want = want; l.pkey = pk; l.ptie = pt;
					done = l.hist[d] == want;             // all that is left of the digit wins: the bytes below stay zero
				}
				l.done = done ? 1u : 0u;
			}
			__syncthreads();
			first = false;
			pkey = l.pkey; ptie = l.ptie;
			if(l.done){ break; }                          // (uniform)
		}
		const uint32_t cnt = min(l.eligible, a.k);

		// the winners, then their order
		if(tid == 0){ l.n = 0; }
		__syncthreads();
		neighbors_visit(a, row, col_a, bits_a, [&](uint32_t j, unsigned long long key) {
			if(neighbors_wins(key, neighbors_tie(a.tie_bytes, j), pkey, ptie)){
				const uint32_t at = atomicAdd(&l.n, 1u);
				if(at < cnt){ l.wkey[at] = key; l.windex[at] = j; }      // (composites are distinct: exactly cnt win)
			}
		});
		uint32_t P = 1;
		while(P < cnt){ P <<= 1; }
		for(uint32_t t = cnt + tid; t < P; t += NEIGHBORS_THREADS){ l.wkey[t] = 0; l.windex[t] = NEIGHBORS_NO_INDEX; }    // behind every winner
		__syncthreads();
		for(uint32_t size = 2; size <= P; size <<= 1){
			for(uint32_t stride = size >> 1; stride > 0; stride >>= 1){
				for(uint32_t t = tid; t < P/2; t += NEIGHBORS_THREADS){
					const uint32_t lo = 2*t - (t & (stride - 1)), hi = lo + stride;
					const bool asc = (lo & size) == 0;
					const unsigned long long xk = l.wkey[lo], yk = l.wkey[hi];
					const uint32_t xi = l.windex[lo], yi = l.windex[hi];
					if(neighbors_behind(xk, xi, yk, yi) == asc){ l.wkey[lo] = yk; l.windex[lo] = yi; l.wkey[hi] = xk; l.windex[hi] = xi; }
				}
				__syncthreads();
			}
		}
		kwage_neighbor *out = a.out + i*a.k;
		for(uint32_t r = tid; r < a.k; r += NEIGHBORS_THREADS){
			kwage_neighbor rec = {NEIGHBORS_NO_INDEX, 0u, 0u, 0u};
			if(r < cnt){
				const uint32_t j = l.windex[r];
				rec.index = j; rec.shared = row[j]; rec.bits_a = bits_a; rec.bits_b = a.bits_b[a.col_b[j]];
			}
			out[r] = rec;
		}
		if(tid == 0){ a.counts[i] = cnt; }
		__syncthreads();                                  // (the LDS is reused by the next entry)
	}
}

}  // namespace kwage

#endif
