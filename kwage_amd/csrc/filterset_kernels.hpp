// kwage_amd/csrc/filterset_kernels.hpp -- gfx950 kernels of the filter set (kwage_filterset, include/kwage_amd.h):
// query Bloom filters turned into ascending row lists on the device.  Included by filterset.hip only.
//
//   column_bits_kernel    one lane per row reads the byte of a column of a group's matrix; the wave's ballot of the
//                         column's bit is one 64-bit word of the packed filter (2^L bits, LSB first)
//   filter_count_kernel   popcount of every word, one sum per workgroup of FS_THREADS words
//   filter_scan_kernel    ONE looping workgroup: exclusive prefix sums of the block sums over all filters (the row
//                         lists lie one after another), then every filter's offset and total
//   filter_expand_kernel  every word writes the indices of its set bits at its offset, lowest first: the list of a
//                         filter ascends, and is the same whatever the launch looked like
//   identity_rows_kernel  the row list 0, 1, .. of a full filter (kwage_group_column_bits)
//
// A packed filter is `words` = max(1, 2^L / 64) words; with fewer than 64 rows the high bits of its one word are 0.
// Workgroup w of the count and expand launches owns words [j*FS_THREADS, (j+1)*FS_THREADS) of filter f, where
// f = w / blocks_per_filter and j = w % blocks_per_filter.
#ifndef KWAGE_AMD_FILTERSET_KERNELS_HPP
#define KWAGE_AMD_FILTERSET_KERNELS_HPP

namespace kwage {

static constexpr uint32_t FS_WAVE = 64;
static constexpr uint32_t FS_THREADS = 256;          // words per workgroup of the count and expand launches
static constexpr uint32_t FS_SCAN_THREADS = 256;     // block sums per round of the scan's one workgroup

struct FilterArgs {
	const unsigned long long *vec;      // [n][words] packed filters
	unsigned long long words;           // per filter
	uint32_t blocks_per_filter;         // ceil(words / FS_THREADS)
	uint32_t n;                         // filters
	uint32_t *sums;                     // [n*blocks_per_filter] set bits per workgroup
	unsigned long long *offs;           // [n*blocks_per_filter + 1] their exclusive prefix sums
	unsigned long long *prefix;         // [n + 1] first entry of every filter's list
	uint32_t *counts;                   // [n] set bits per filter
	uint32_t *rows;                     // [offs[n*blocks_per_filter]] the lists
};

// Inclusive prefix sum over the lanes of a wave.
template <typename T>
__device__ __forceinline__ T fs_wave_incl_scan(T v)
{
	const uint32_t lane = threadIdx.x & (FS_WAVE - 1);
#pragma unroll
	for(int d = 1; d < (int)FS_WAVE; d <<= 1){
		const T up = __shfl_up(v, d);
		if((int)lane >= d){ v += up; }
	}
	return v;
}

// cols[q]: a global column of the matrix; grid: n * ceil(nrows / FS_THREADS) workgroups, filter-major.
__global__ __launch_bounds__(FS_THREADS) void column_bits_kernel(const uint8_t *db, unsigned long long stride, unsigned long long nrows,
                                                                 const unsigned long long *cols, uint32_t blocks_per_col,
                                                                 unsigned long long words, unsigned long long *vec)
{
	const uint32_t q = blockIdx.x / blocks_per_col, j = blockIdx.x % blocks_per_col;
	const unsigned long long c = cols[q];
	const unsigned long long row = (unsigned long long)j*FS_THREADS + threadIdx.x;
	bool bit = false;
	if(row < nrows){ bit = ((db[row*stride + (c >> 3)] >> (c & 7u)) & 1u) != 0; }
	const unsigned long long word = __ballot(bit);
	// (a wave's first row is a multiple of 64: it is the wave's word index times 64; rows past the end ballot 0)
	if((threadIdx.x & (FS_WAVE - 1)) == 0 && row < nrows){ vec[(unsigned long long)q*words + (row >> 6)] = word; }
}

__global__ __launch_bounds__(FS_THREADS) void filter_count_kernel(FilterArgs a)
{
	__shared__ uint32_t wave_sum[FS_THREADS/FS_WAVE];
	const uint32_t f = blockIdx.x / a.blocks_per_filter, j = blockIdx.x % a.blocks_per_filter;
	const unsigned long long w = (unsigned long long)j*FS_THREADS + threadIdx.x;
	uint32_t c = (w < a.words) ? (uint32_t)__popcll(a.vec[(unsigned long long)f*a.words + w]) : 0u;
#pragma unroll
	for(int d = FS_WAVE/2; d >= 1; d >>= 1){ c += __shfl_xor(c, d); }
	if((threadIdx.x & (FS_WAVE - 1)) == 0){ wave_sum[threadIdx.x >> 6] = c; }
	__syncthreads();
	if(threadIdx.x == 0){
		uint32_t t = 0;
#pragma unroll
		for(uint32_t k = 0; k < FS_THREADS/FS_WAVE; ++k){ t += wave_sum[k]; }
		a.sums[blockIdx.x] = t;
	}
}

// One workgroup.  Round after round of FS_SCAN_THREADS block sums: a scan within every wave, the waves' totals through
// LDS, the rounds before it in `carry`.
__global__ __launch_bounds__(FS_SCAN_THREADS) void filter_scan_kernel(FilterArgs a)
{
	constexpr uint32_t WAVES = FS_SCAN_THREADS/FS_WAVE;
	__shared__ unsigned long long wave_tot[WAVES];
	const unsigned long long items = (unsigned long long)a.n*a.blocks_per_filter;
	const uint32_t lane = threadIdx.x & (FS_WAVE - 1), wv = threadIdx.x >> 6;
	unsigned long long carry = 0;
	for(unsigned long long base = 0; base < items; base += FS_SCAN_THREADS){
		const unsigned long long i = base + threadIdx.x;
		const unsigned long long v = (i < items) ? a.sums[i] : 0ull;
		const unsigned long long incl = fs_wave_incl_scan(v);
		if(lane == FS_WAVE - 1){ wave_tot[wv] = incl; }
		__syncthreads();
		unsigned long long before = 0, total = 0;
#pragma unroll
		for(uint32_t k = 0; k < WAVES; ++k){
			const unsigned long long t = wave_tot[k];
			if(k < wv){ before += t; }
			total += t;
		}
		if(i < items){ a.offs[i] = carry + before + incl - v; }
		carry += total;
		__syncthreads();            // (wave_tot is rewritten by the next round)
	}
	if(threadIdx.x == 0){ a.offs[items] = carry; }
	// the offsets written above are read below by other lanes of this workgroup
	__threadfence();
	__syncthreads();
	for(uint32_t f = threadIdx.x; f <= a.n; f += FS_SCAN_THREADS){
		const unsigned long long at = a.offs[(unsigned long long)f*a.blocks_per_filter];
		a.prefix[f] = at;
		if(f < a.n){ a.counts[f] = (uint32_t)(a.offs[(unsigned long long)(f + 1)*a.blocks_per_filter] - at); }
	}
}

__global__ __launch_bounds__(FS_THREADS) void filter_expand_kernel(FilterArgs a)
{
	__shared__ uint32_t wave_tot[FS_THREADS/FS_WAVE];
	const uint32_t f = blockIdx.x / a.blocks_per_filter, j = blockIdx.x % a.blocks_per_filter;
	const unsigned long long w = (unsigned long long)j*FS_THREADS + threadIdx.x;
	unsigned long long word = (w < a.words) ? a.vec[(unsigned long long)f*a.words + w] : 0ull;
	const uint32_t c = (uint32_t)__popcll(word);
	const uint32_t incl = fs_wave_incl_scan(c);
	if((threadIdx.x & (FS_WAVE - 1)) == FS_WAVE - 1){ wave_tot[threadIdx.x >> 6] = incl; }
	__syncthreads();
	uint32_t before = 0;
#pragma unroll
	for(uint32_t k = 0; k < FS_THREADS/FS_WAVE; ++k){ if(k < (threadIdx.x >> 6)){ before += wave_tot[k]; } }
	// the word's c entries: [at, at + c), inside the workgroup's [offs[blockIdx.x], offs[blockIdx.x + 1])
	unsigned long long at = a.offs[blockIdx.x] + before + incl - c;
	const uint32_t row0 = (uint32_t)(w << 6);
	while(word){
		a.rows[at++] = row0 + (uint32_t)__builtin_ctzll(word);
		word &= word - 1;
	}
}

__global__ __launch_bounds__(FS_THREADS) void identity_rows_kernel(uint32_t *rows, unsigned long long n)
{
	const unsigned long long step = (unsigned long long)gridDim.x*FS_THREADS;
	for(unsigned long long i = (unsigned long long)blockIdx.x*FS_THREADS + threadIdx.x; i < n; i += step){ rows[i] = (uint32_t)i; }
}

}  // namespace kwage

#endif
