// kwage_amd/csrc/topk_merge_kernels.hpp -- gfx950 kernels of kwage_topk_merge_device: several top-k lists (any number
// of kwage_hit records, unordered) merged to the first k records per query under (num_match descending, order[column]
// ascending).  Included by topk_merge.hip only.
//
//   merge_count_kernel    per-query histogram of the input (global atomics on n_queries counters, one per run of equal
//                         queries in a wave); records with a query
//                         or column outside the tables are counted in `bad` and otherwise ignored
//   merge_scan_kernel     one workgroup: exclusive prefix sums of the bucket sizes and of min(k, bucket) -- the output
//                         offsets, known before any selection -- and the output total; resets the counters to 0
//   merge_scatter_kernel  every record to its query's bucket as a 64-bit key score << 32 | ~order[column], plus its column
//   merge_select_kernel   one workgroup per query (the grid loops over the queries): 8-bit radix select of the k-th largest key of the bucket (keys are
//                         distinct: an exact cut), the <= k winners into LDS, bitonic sort by column, written at the
//                         query's output offset (records at or beyond the capacity are not written)
#ifndef KWAGE_AMD_TOPK_MERGE_KERNELS_HPP
#define KWAGE_AMD_TOPK_MERGE_KERNELS_HPP

namespace kwage {

static constexpr uint32_t TM_WAVE = 64;
static constexpr uint32_t TM_SCAN_THREADS = 1024;

struct MergeArgs {
	const kwage_hit *hits;
	unsigned long long n_hits;
	uint32_t n_queries;
	uint32_t k;
	const uint32_t *order;              // tie key per column, or NULL (the column itself)
	unsigned long long n_order;
	uint32_t *bucket_n;                 // [n_queries]: histogram, then (reset by the scan) the scatter's fill cursor
	uint32_t *bucket_off;               // [n_queries + 1]
	unsigned long long *out_off;        // [n_queries + 1]
	unsigned long long *keys;           // [n_hits] bucketed keys
	uint32_t *cols;                     // [n_hits] their columns
	unsigned long long *bad;            // records outside the tables
	kwage_hit *out;
	unsigned long long out_capacity;
	unsigned long long *out_count;      // the caller's device word: the output total
};

__device__ __forceinline__ bool merge_record_ok(const MergeArgs &a, const kwage_hit &h)
{
	return h.query < a.n_queries && (!a.order || h.column < a.n_order);
}

// A wave's 64 consecutive records, as the count and scatter passes see them: the lists arrive with each query's records
// in runs (a source's list is ordered by query), so the lanes of a run share ONE atomic on their query's counter.
// key: the record's query, or TM_NONE for a record outside the tables or past the end (valid queries are < 2^31).
static constexpr uint32_t TM_NONE = 0xFFFFFFFFu;
struct WaveRun {
	uint32_t key;       // this lane's query, or TM_NONE
	uint32_t leader;    // the lane that starts this lane's run
	uint32_t len;       // on a leader: the run's length (lanes leader .. leader + len - 1)
	bool head;
};

__device__ __forceinline__ WaveRun wave_runs(uint32_t key)
{
	const uint32_t lane = threadIdx.x & (TM_WAVE - 1);
	const uint32_t prev = __shfl_up(key, 1);
	WaveRun r;
	r.key = key;
	r.head = (lane == 0) || (key != prev);
	const unsigned long long heads = __ballot(r.head);
	const unsigned long long upto = (2ull << lane) - 1ull;              // lanes 0 .. lane (all 64 at lane 63)
	r.leader = 63u - (uint32_t)__clzll(heads & upto);
	const unsigned long long after = heads & ~upto;
	r.len = (after ? (uint32_t)(__ffsll((long long)after) - 1) : TM_WAVE) - lane;
	return r;
}

// The grid-stride loop runs per WAVE (blockDim and the stride are multiples of 64): every lane of a wave takes part in
// every step, so the shuffles and ballots of wave_runs see all 64 lanes.
__global__ __launch_bounds__(256) void merge_count_kernel(MergeArgs a)
{
	const uint32_t lane = threadIdx.x & (TM_WAVE - 1);
	const unsigned long long stride = (unsigned long long)gridDim.x*blockDim.x;
	uint32_t bad = 0;
	for(unsigned long long w0 = (unsigned long long)blockIdx.x*blockDim.x + (threadIdx.x - lane); w0 < a.n_hits; w0 += stride){
		const unsigned long long i = w0 + lane;
		uint32_t key = TM_NONE;
		if(i < a.n_hits){
			const kwage_hit h = a.hits[i];
			if(merge_record_ok(a, h)){ key = h.query; } else { ++bad; }
		}
		const WaveRun r = wave_runs(key);
		if(r.head && r.key != TM_NONE){ atomicAdd(&a.bucket_n[r.key], r.len); }
	}
	if(bad){ atomicAdd(a.bad, (unsigned long long)bad); }
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ unsigned long long tm_wave_incl_scan(unsigned long long v)
{
	const uint32_t lane = threadIdx.x & (TM_WAVE - 1);
#pragma unroll
	for(uint32_t d = 1; d < TM_WAVE; d <<= 1){
		const unsigned long long up = __shfl_up(v, d);
		if(lane >= d){ v += up; }
	}
	return v;
}

// exclusive prefix over the workgroup's threads of (x, y); *tot_x / *tot_y receive the sums
__device__ __forceinline__ void tm_block_excl_scan(unsigned long long &x, unsigned long long &y, unsigned long long *tot_x, unsigned long long *tot_y)
{
	__shared__ unsigned long long wx[TM_SCAN_THREADS/TM_WAVE], wy[TM_SCAN_THREADS/TM_WAVE];
	const uint32_t lane = threadIdx.x & (TM_WAVE - 1), w = threadIdx.x/TM_WAVE, nw = blockDim.x/TM_WAVE;
	const unsigned long long ix = tm_wave_incl_scan(x), iy = tm_wave_incl_scan(y);
	if(lane == TM_WAVE - 1){ wx[w] = ix; wy[w] = iy; }
	__syncthreads();
	unsigned long long bx = 0, by = 0, sx = 0, sy = 0;
	for(uint32_t i = 0; i < nw; ++i){
		if(i < w){ bx += wx[i]; by += wy[i]; }
		sx += wx[i];
		sy += wy[i];
	}
	x = bx + ix - x;
	y = by + iy - y;
	*tot_x = sx;
	*tot_y = sy;
}

// One workgroup of TM_SCAN_THREADS: thread t owns the queries [t*per, (t+1)*per).
__global__ __launch_bounds__(TM_SCAN_THREADS) void merge_scan_kernel(MergeArgs a)
{
	const uint32_t n = a.n_queries;
	const uint32_t per = (n + TM_SCAN_THREADS - 1)/TM_SCAN_THREADS;
	const uint32_t q0 = min(n, threadIdx.x*per), q1 = min(n, q0 + per);
	unsigned long long sb = 0, so = 0;
	for(uint32_t q = q0; q < q1; ++q){ const uint32_t c = a.bucket_n[q]; sb += c; so += min(c, a.k); }
	unsigned long long tb, to;
	tm_block_excl_scan(sb, so, &tb, &to);
	for(uint32_t q = q0; q < q1; ++q){
		const uint32_t c = a.bucket_n[q];
		a.bucket_off[q] = (uint32_t)sb;
		a.out_off[q] = so;
		a.bucket_n[q] = 0;
		sb += c;
		so += min(c, a.k);
	}
	if(threadIdx.x == 0){
		a.bucket_off[n] = (uint32_t)tb;
		a.out_off[n] = to;
		*a.out_count = to;
	}
}

__global__ __launch_bounds__(256) void merge_scatter_kernel(MergeArgs a)
{
	const uint32_t lane = threadIdx.x & (TM_WAVE - 1);
	const unsigned long long stride = (unsigned long long)gridDim.x*blockDim.x;
	for(unsigned long long w0 = (unsigned long long)blockIdx.x*blockDim.x + (threadIdx.x - lane); w0 < a.n_hits; w0 += stride){
		const unsigned long long i = w0 + lane;
		kwage_hit h = {0, 0, 0};
		uint32_t key = TM_NONE;
		if(i < a.n_hits){
			h = a.hits[i];
			if(merge_record_ok(a, h)){ key = h.query; }
		}
		const WaveRun r = wave_runs(key);
		uint32_t first = 0;                               // the run's first slot in its bucket (on the leader)
		if(r.head && r.key != TM_NONE){ first = a.bucket_off[r.key] + atomicAdd(&a.bucket_n[r.key], r.len); }
		first = __shfl(first, (int)r.leader);
		if(r.key != TM_NONE){
			const uint32_t tie = a.order ? a.order[h.column] : h.column;
			const uint32_t at = first + (lane - r.leader);
			a.keys[at] = ((unsigned long long)h.num_match << 32) | (unsigned long long)(~tie);
			a.cols[at] = h.column;
		}
	}
}

__host__ __device__ __forceinline__ uint32_t tm_pow2(uint32_t n)
{
	uint32_t p = 1;
	while(p < n){ p <<= 1; }
	return p;
}

struct SelectLds {
	uint32_t hist[256];
	unsigned long long prefix;
	uint32_t want, n;
};

// One query's selection by a workgroup of BLOCK threads (every thread calls it; q is uniform).
template <uint32_t BLOCK>
__device__ __forceinline__ void merge_select_query(const MergeArgs &a, uint32_t q, unsigned long long *win, SelectLds &l)
{
	uint32_t *hist = l.hist;
	const uint32_t tid = threadIdx.x;
	const uint32_t b0 = a.bucket_off[q], m = a.bucket_off[q + 1] - b0;
	if(m == 0){ return; }                                 // uniform per workgroup
	const uint32_t k = a.k;
	const uint32_t cnt = min(m, k);
	const unsigned long long *kq = a.keys + b0;
	const uint32_t *cq = a.cols + b0;

	unsigned long long thr = 0;                           // keys >= thr win (all of them when m <= k)
	if(m > k){
		unsigned long long prefix = 0, mask = 0;
		uint32_t want = k;                                // rank from the top of the k-th largest key among those matching prefix
		for(int shift = 56; shift >= 0; shift -= 8){
			for(uint32_t i = tid; i < 256; i += BLOCK){ hist[i] = 0; }
			__syncthreads();
			for(uint32_t j = tid; j < m; j += BLOCK){
				const unsigned long long key = kq[j];
				if((key & mask) == prefix){ atomicAdd(&hist[(key >> shift) & 255u], 1u); }
			}
			__syncthreads();
			if(tid == 0){
				uint32_t above = 0;
				int b = 255;
				for(; b > 0 && above + hist[b] < want; --b){ above += hist[b]; }
				l.want = want - above;
				l.prefix = prefix | ((unsigned long long)b << shift);
			}
			__syncthreads();
			want = l.want;
			prefix = l.prefix;
			mask |= 255ull << shift;
		}
		thr = prefix;                                     // distinct keys: exactly k are >= the k-th largest
	}

	if(tid == 0){ l.n = 0; }
	__syncthreads();
	for(uint32_t j = tid; j < m; j += BLOCK){
		const unsigned long long key = kq[j];
		if(key >= thr){
			const uint32_t at = atomicAdd(&l.n, 1u);
			if(at < cnt){ win[at] = ((unsigned long long)cq[j] << 32) | (key >> 32); }     // (a duplicate key cannot overflow win)
		}
	}
	const uint32_t P = tm_pow2(cnt);
	for(uint32_t i = cnt + tid; i < P; i += BLOCK){ win[i] = ~0ull; }
	__syncthreads();
	// bitonic sort of win[0, P) ascending: by column (columns of one query are distinct)
	for(uint32_t size = 2; size <= P; size <<= 1){
		for(uint32_t stride = size >> 1; stride > 0; stride >>= 1){
			for(uint32_t t = tid; t < P/2; t += BLOCK){
				const uint32_t lo = 2*t - (t & (stride - 1)), hi = lo + stride;
				const bool asc = (lo & size) == 0;
				const unsigned long long x = win[lo], y = win[hi];
				if((x > y) == asc){ win[lo] = y; win[hi] = x; }
			}
			__syncthreads();
		}
	}
	const unsigned long long o = a.out_off[q];
	for(uint32_t i = tid; i < cnt; i += BLOCK){
		if(o + i >= a.out_capacity){ break; }
		const unsigned long long v = win[i];
		kwage_hit h;
		h.query = q;
		h.column = (uint32_t)(v >> 32);
		h.num_match = (uint32_t)v;
		a.out[o + i] = h;
	}
}

// A workgroup of BLOCK threads per query, the grid looping over the queries (any count fits one launch); dynamic LDS of
// tm_pow2(k) x 8 bytes.
template <uint32_t BLOCK>
__global__ __launch_bounds__(BLOCK) void merge_select_kernel(MergeArgs a)
{
	extern __shared__ unsigned long long win[];           // (column << 32 | num_match) of the winners: tm_pow2(k) slots
	__shared__ SelectLds l;
	for(uint32_t q = blockIdx.x; q < a.n_queries; q += gridDim.x){
		merge_select_query<BLOCK>(a, q, win, l);
		__syncthreads();                                  // (the LDS is reused by the next query)
	}
}

}  // namespace kwage

#endif
