// kwage_amd/csrc/filterset.hip -- the filter set and the filter search (include/kwage_amd.h): whole Bloom filters as
// the questions of a search.  No counterpart in the reference.
//
//   a column of a group / host bits  ->  packed filter  ->  filter_count_kernel -> filter_scan_kernel -> filter_expand_kernel
//                                                           = the filter's set rows, ascending: a row list
//   row lists  ->  the score stage of the dense score search (score_stage.hpp, defined in scores.hip) with ONE row per
//                  entry: cell (i, c) = rows set in both filter i and column c
//
// This unit owns the kernels of filterset_kernels.hpp and none of the score kernels: the stage it calls runs the
// instantiations scores.hip already has for one hash function.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "kwage_amd.h"
#include "engine_state.hpp"
#include "pool_blocks.hpp"
#include "score_stage.hpp"
#include "filterset_kernels.hpp"

// n filters over 2^L rows: one concatenated row list, each filter's rows ascending.  The three device arrays are blocks
// of the context's pool and go back to it when the set is destroyed.
struct kwage_filterset {
	kwage_ctx *ctx = nullptr;
	kwage_params params{};
	uint32_t n = 0;
	uint64_t total = 0;                 // entries of the row list
	uint32_t max_count = 0;
	kwage::DevPool::Block rows{nullptr, 0}, prefix{nullptr, 0}, counts{nullptr, 0};
	std::vector<uint32_t> h_counts;     // n
	std::vector<uint64_t> h_prefix;     // n + 1
	~kwage_filterset()
	{
		if(!ctx){ return; }
		ctx->batch_pool.give(rows.p, rows.cap);
		ctx->batch_pool.give(prefix.p, prefix.cap);
		ctx->batch_pool.give(counts.p, counts.cap);
	}
};

namespace kwage {
namespace {

thread_local char last_kernel[64] = "";

int take_kept(kwage_ctx *ctx, uint64_t bytes, DevPool::Block *b)
{
	HIP_TRY(ctx->batch_pool.take(bytes, &b->p, &b->cap));
	return KWAGE_OK;
}

bool same_params(const kwage_params &a, const kwage_params &b)
{
	return a.kmer_len == b.kmer_len && a.num_hash == b.num_hash && a.log_2_filter_len == b.log_2_filter_len && a.hash_func == b.hash_func;
}

uint64_t words_of(const kwage_params &p) { return std::max<uint64_t>(1, (1ull << p.log_2_filter_len)/64); }

// What both sources refuse before anything is allocated.
int filterset_check(const kwage_params &p, uint32_t n, const char *what)
{
	int rc;
	if((rc = check_params(&p))){ return rc; }
	if(p.log_2_filter_len >= 32){
		return fail(KWAGE_ERR_ARG, "%s: a filter of 2^32 rows is not supported (the set-bit count of a full one does not fit 32 bits)", what);
	}
	const uint64_t blocks = (words_of(p) + FS_THREADS - 1)/FS_THREADS;
	const uint64_t row_blocks = ((1ull << p.log_2_filter_len) + FS_THREADS - 1)/FS_THREADS;
	if((uint64_t)n*std::max(blocks, row_blocks) > 0x7FFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: too many filters for one launch", what); }
	return KWAGE_OK;
}

// From the packed filters ([n][words] on the device) to the set's row lists.  Queued on the context's first stream and
// waited for; `fs` owns what is kept, `blocks` what is not.
int filterset_build(kwage_filterset *fs, const unsigned long long *d_vec, PoolBlocks &blocks)
{
	int rc;
	kwage_ctx *ctx = fs->ctx;
	hipStream_t s = ctx->stream;
	const uint32_t n = fs->n;
	fs->h_counts.assign(n, 0);
	fs->h_prefix.assign((size_t)n + 1, 0);
	if(!n){ return KWAGE_OK; }
	FilterArgs a;
	memset(&a, 0, sizeof(a));
	a.vec = d_vec;
	a.words = words_of(fs->params);
	a.blocks_per_filter = (uint32_t)((a.words + FS_THREADS - 1)/FS_THREADS);
	a.n = n;
	const uint64_t items = (uint64_t)n*a.blocks_per_filter;          // (<= 2^31 - 1: filterset_check)
	if((rc = blocks.take(items*sizeof(uint32_t), &a.sums))){ return rc; }
	if((rc = blocks.take((items + 1)*sizeof(uint64_t), &a.offs))){ return rc; }
	if((rc = take_kept(ctx, ((uint64_t)n + 1)*sizeof(uint64_t), &fs->prefix))){ return rc; }
	if((rc = take_kept(ctx, (uint64_t)n*sizeof(uint32_t), &fs->counts))){ return rc; }
	a.prefix = (unsigned long long*)fs->prefix.p;
	a.counts = (uint32_t*)fs->counts.p;
	hipLaunchKernelGGL(filter_count_kernel, dim3((uint32_t)items), dim3(FS_THREADS), 0, s, a);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(FS_SCAN_THREADS), 0, s, a);
	HIP_TRY(hipGetLastError());
	// the totals: the host needs them for the list's size, the launch plan of a search and the counters' width
	HIP_TRY(hipMemcpyAsync(fs->h_counts.data(), a.counts, (size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	for(uint32_t i = 0; i < n; ++i){
		fs->h_prefix[i + 1] = fs->h_prefix[i] + fs->h_counts[i];
		fs->max_count = std::max(fs->max_count, fs->h_counts[i]);
	}
	fs->total = fs->h_prefix[n];
	if((rc = take_kept(ctx, std::max<uint64_t>(fs->total, 1)*sizeof(uint32_t), &fs->rows))){ return rc; }
	a.rows = (uint32_t*)fs->rows.p;
	hipLaunchKernelGGL(filter_expand_kernel, dim3((uint32_t)items), dim3(FS_THREADS), 0, s, a);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	return KWAGE_OK;
}

int from_columns(kwage_group *g, const uint64_t *columns, uint32_t n, kwage_filterset *fs, PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_filterset_from_columns";
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "%s: kwage_group_finalize() must be called first", what); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group does not hold whole filters", what); }
	if((rc = filterset_check(g->params, n, what))){ return rc; }
	const uint64_t span = g->next_byte*8;
	for(uint32_t i = 0; i < n; ++i){
		const uint64_t c = columns[i];
		if(c >= span){ return fail(KWAGE_ERR_ARG, "%s: column %llu is beyond the group's span %llu", what, (unsigned long long)c, (unsigned long long)span); }
		if(!((g->h_valid[c/8] >> (c%8)) & 1u)){ return fail(KWAGE_ERR_ARG, "%s: column %llu is a pad column", what, (unsigned long long)c); }
	}
	kwage_ctx *ctx = g->ctx;
	if((rc = set_device(ctx))){ return rc; }
	fs->ctx = ctx;
	fs->params = g->params;
	fs->n = n;
	unsigned long long *d_vec = nullptr, *d_cols = nullptr;
	const uint64_t words = words_of(g->params);
	if(n){
		hipStream_t s = ctx->stream;
		if((rc = blocks.take((uint64_t)n*words*sizeof(uint64_t), &d_vec))){ return rc; }
		if((rc = blocks.take((uint64_t)n*sizeof(uint64_t), &d_cols))){ return rc; }
		HIP_TRY(hipMemcpyAsync(d_cols, columns, (size_t)n*sizeof(uint64_t), hipMemcpyHostToDevice, s));
		const uint32_t blocks_per_col = (uint32_t)((g->nrows + FS_THREADS - 1)/FS_THREADS);
		hipLaunchKernelGGL(column_bits_kernel, dim3(n*blocks_per_col), dim3(FS_THREADS), 0, s, g->d_bits, (unsigned long long)g->stride,
		                   (unsigned long long)g->nrows, d_cols, blocks_per_col, (unsigned long long)words, d_vec);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(s));          // (`columns` is the caller's: the copy above is done when this call returns)
	}
	return filterset_build(fs, d_vec, blocks);
}

int from_bits(kwage_ctx *ctx, const kwage_params *params, const void *bits, uint64_t filter_stride_bytes, uint32_t n, kwage_filterset *fs,
              PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_filterset_from_bits";
	if((rc = filterset_check(*params, n, what))){ return rc; }
	const uint64_t nrows = 1ull << params->log_2_filter_len;
	const uint64_t filter_bytes = std::max<uint64_t>(1, nrows/8), words = words_of(*params);
	if(n && !bits){ return fail(KWAGE_ERR_ARG, "%s: bits is NULL", what); }
	if(n > 1 && filter_stride_bytes < filter_bytes){
		return fail(KWAGE_ERR_ARG, "%s: filter_stride_bytes %llu is below the %llu bytes of a filter", what, (unsigned long long)filter_stride_bytes,
		            (unsigned long long)filter_bytes);
	}
	if((rc = set_device(ctx))){ return rc; }
	fs->ctx = ctx;
	fs->params = *params;
	fs->n = n;
	unsigned long long *d_vec = nullptr;
	if(n){
		hipStream_t s = ctx->stream;
		if((rc = blocks.take((uint64_t)n*words*sizeof(uint64_t), &d_vec))){ return rc; }
		const unsigned char *src = (const unsigned char*)bits;
		if(nrows < 64){
			// fewer rows than a word has bits: the words are made here, bits at or beyond 2^L dropped
			std::vector<unsigned long long> w(n, 0);
			for(uint32_t i = 0; i < n; ++i){
				unsigned long long x = 0;
				memcpy(&x, src + (uint64_t)i*filter_stride_bytes, (size_t)filter_bytes);       // (little endian, like every file format here)
				w[i] = x & ((1ull << nrows) - 1);
			}
			HIP_TRY(hipMemcpyAsync(d_vec, w.data(), (size_t)n*sizeof(uint64_t), hipMemcpyHostToDevice, s));
			HIP_TRY(hipStreamSynchronize(s));
		}
		else{
			HIP_TRY(hipMemcpy2DAsync(d_vec, filter_bytes, src, (n > 1) ? filter_stride_bytes : filter_bytes, filter_bytes, n, hipMemcpyHostToDevice, s));
			HIP_TRY(hipStreamSynchronize(s));
		}
	}
	return filterset_build(fs, d_vec, blocks);
}

// What a filter search refuses on the host.
int filter_scores_check(kwage_group *g, kwage_filterset *fs, uint64_t row_elems, const char *what)
{
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "kwage_group_finalize() must be called before searching"); }
	if(fs->ctx != g->ctx){ return fail(KWAGE_ERR_ARG, "%s: filter set and group belong to different contexts", what); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group does not hold the rows of a whole filter", what); }
	if(!same_params(g->params, fs->params)){
		return fail(KWAGE_ERR_ARG, "%s: the filter set (k %u, %u hash functions, 2^%u rows, hash %d) and the group (k %u, %u, 2^%u, %d) were built "
		            "with different parameters: their filters are not comparable", what, fs->params.kmer_len, fs->params.num_hash,
		            fs->params.log_2_filter_len, fs->params.hash_func, g->params.kmer_len, g->params.num_hash, g->params.log_2_filter_len,
		            g->params.hash_func);
	}
	const uint64_t span = g->next_byte*8;
	if(row_elems < span || row_elems % 4 != 0){
		return fail(KWAGE_ERR_ARG, "%s: row_elems must be a multiple of 4 and at least the group's column span %llu (got %llu)", what,
		            (unsigned long long)span, (unsigned long long)row_elems);
	}
	return KWAGE_OK;
}

int filter_scores_device(kwage_group *g, kwage_filterset *fs, void *scores_dev, uint64_t row_elems, uint32_t flags, float *ms,
                         PoolBlocks &blocks, const char *what)
{
	int rc;
	last_kernel[0] = 0;
	if(ms){ *ms = 0; }
	if((rc = filter_scores_check(g, fs, row_elems, what))){ return rc; }
	if(fs->n && g->next_byte && (!scores_dev || ((uintptr_t)scores_dev & 15u))){
		return fail(KWAGE_ERR_ARG, "%s: the score matrix must be a 16-byte aligned device pointer", what);
	}
	if((rc = set_device(g->ctx))){ return rc; }
	TilePlan plan;
	if((rc = score_stage_plan(g, fs->n, fs->max_count, &plan))){ return rc; }
	// one row per entry, whatever the group's hash count: the list IS the filter's set rows
	const RowListView v = {(const uint32_t*)fs->rows.p, (const uint64_t*)fs->prefix.p, (const uint32_t*)fs->counts.p, fs->n, fs->max_count, 1};
	ScoreArgs sa;
	sa.out = (uint32_t*)scores_dev;
	sa.row_elems = row_elems;
	sa.span = 0;
	sa.form = SCORES_FORM_WAVE;
	return score_stage_run(g, v, plan, sa, flags, ms, blocks, last_kernel);
}

int filter_scores_host(kwage_group *g, kwage_filterset *fs, uint32_t *scores, uint64_t row_elems, uint32_t flags, float *ms, PoolBlocks &blocks)
{
	int rc;
	static const char *what = "kwage_search_filter_scores";
	if((rc = filter_scores_check(g, fs, row_elems, what))){ return rc; }
	rc = scores_to_host(g, fs->n, scores, row_elems, blocks, what, [&](uint32_t *d_scores, uint64_t span) {
		return filter_scores_device(g, fs, d_scores, span, flags, ms, blocks, what);
	});
	if(rc){ return rc; }
	if(fs->n && g->next_byte){ HIP_TRY(hipStreamSynchronize(g->ctx->stream)); }
	return KWAGE_OK;
}

// Every column's set-bit count: the score stage over the identity row list (every row once), one row of cells.
int column_bits_device(kwage_group *g, void *out_dev, PoolBlocks &blocks, const char *what)
{
	int rc;
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "%s: kwage_group_finalize() must be called first", what); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group does not hold whole columns", what); }
	if(g->params.log_2_filter_len >= 32){ return fail(KWAGE_ERR_ARG, "%s: a column of 2^32 rows may hold more set bits than 32 bits count", what); }
	const uint64_t span = g->next_byte*8;
	if(span && (!out_dev || ((uintptr_t)out_dev & 15u))){ return fail(KWAGE_ERR_ARG, "%s: the counts must go to a 16-byte aligned device pointer", what); }
	if(!span){ return KWAGE_OK; }
	kwage_ctx *ctx = g->ctx;
	if((rc = set_device(ctx))){ return rc; }
	const uint64_t nrows = g->nrows;
	TilePlan plan;
	if((rc = score_stage_plan(g, 1, nrows, &plan))){ return rc; }
	void *p = nullptr;
	uint64_t cap = 0;
	if(ctx->batch_pool.take(nrows*sizeof(uint32_t) + 64, &p, &cap) != hipSuccess){
		(void)hipGetLastError();
		return fail(KWAGE_ERR_DEVICE, "%s: the identity row list (%llu rows, %llu bytes) could not be allocated on the device", what,
		            (unsigned long long)nrows, (unsigned long long)(nrows*sizeof(uint32_t)));
	}
	blocks.held.push_back(DevPool::Block{p, cap});
	// [pos_off: 2 x u64 | count: u32, pad | rows]
	unsigned long long *d_head = (unsigned long long*)p;
	uint32_t *d_rows = (uint32_t*)((char*)p + 64);
	const unsigned long long head[3] = {0ull, (unsigned long long)nrows, (unsigned long long)nrows};       // (little endian: the low word of head[2] is the count)
	hipStream_t s = ctx->stream;
	HIP_TRY(hipMemcpyAsync(d_head, head, sizeof(head), hipMemcpyHostToDevice, s));
	const uint32_t wgs = (uint32_t)std::min<uint64_t>((nrows + FS_THREADS - 1)/FS_THREADS, 4096);
	hipLaunchKernelGGL(identity_rows_kernel, dim3(wgs), dim3(FS_THREADS), 0, s, d_rows, (unsigned long long)nrows);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));              // (`head` lives on this stack frame)
	const RowListView v = {d_rows, (const uint64_t*)d_head, (const uint32_t*)(d_head + 2), 1, nrows, 1};
	ScoreArgs sa;
	sa.out = (uint32_t*)out_dev;
	sa.row_elems = span;
	sa.span = 0;
	sa.form = SCORES_FORM_WAVE;
	char name[64] = "";
	return score_stage_run(g, v, plan, sa, 0, nullptr, blocks, name);
}

}  // namespace
}  // namespace kwage

extern "C" int kwage_filterset_from_columns(kwage_group *g, const uint64_t *columns, uint32_t n, kwage_filterset **out)
{
	if(!g || !out || (n && !columns)){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_from_columns: NULL argument"); }
	std::unique_ptr<kwage_filterset> fs(new kwage_filterset);
	int rc;
	{
		kwage::PoolBlocks blocks(&g->ctx->batch_pool);
		rc = kwage::settle(g->ctx, kwage::from_columns(g, columns, n, fs.get(), blocks));
	}
	if(rc){ return rc; }
	*out = fs.release();
	return KWAGE_OK;
}

extern "C" int kwage_filterset_from_bits(kwage_ctx *ctx, const kwage_params *params, const void *bits, uint64_t filter_stride_bytes,
                                         uint32_t n, kwage_filterset **out)
{
	if(!ctx || !params || !out){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_from_bits: NULL argument"); }
	std::unique_ptr<kwage_filterset> fs(new kwage_filterset);
	int rc;
	{
		kwage::PoolBlocks blocks(&ctx->batch_pool);
		rc = kwage::settle(ctx, kwage::from_bits(ctx, params, bits, filter_stride_bytes, n, fs.get(), blocks));
	}
	if(rc){ return rc; }
	*out = fs.release();
	return KWAGE_OK;
}

extern "C" void kwage_filterset_destroy(kwage_filterset *fs) { delete fs; }

extern "C" uint32_t kwage_filterset_num_filters(const kwage_filterset *fs) { return fs ? fs->n : 0; }

extern "C" int kwage_filterset_bit_counts(const kwage_filterset *fs, uint32_t *out)
{
	if(!fs || (fs->n && !out)){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_bit_counts: NULL argument"); }
	if(fs->n){ memcpy(out, fs->h_counts.data(), (size_t)fs->n*sizeof(uint32_t)); }
	return KWAGE_OK;
}

extern "C" int kwage_filterset_read_rows(const kwage_filterset *fs, uint32_t i, uint32_t *out, uint64_t capacity, uint64_t *count)
{
	using kwage::fail;
	if(!fs || !count){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_read_rows: NULL argument"); }
	if(i >= fs->n){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_read_rows: filter %u of %u", i, fs->n); }
	const uint64_t c = fs->h_counts[i];
	*count = c;
	const uint64_t take = std::min(c, capacity);
	if(take){
		if(!out){ return kwage::fail(KWAGE_ERR_ARG, "kwage_filterset_read_rows: out is NULL"); }
		int rc;
		if((rc = kwage::set_device(fs->ctx))){ return rc; }
		// the device's own prefix entry addresses the copy: what a search would read
		unsigned long long at = 0;
		HIP_TRY(hipMemcpy(&at, (const unsigned long long*)fs->prefix.p + i, sizeof(at), hipMemcpyDeviceToHost));
		if(at != fs->h_prefix[i]){ return kwage::fail(KWAGE_ERR_STATE, "kwage_filterset_read_rows: the device's prefix %llu differs from the host's %llu", at, (unsigned long long)fs->h_prefix[i]); }
		HIP_TRY(hipMemcpy(out, (const uint32_t*)fs->rows.p + at, (size_t)take*sizeof(uint32_t), hipMemcpyDeviceToHost));
	}
	return KWAGE_OK;
}

extern "C" int kwage_search_filter_scores_device(kwage_group *g, kwage_filterset *fs, void *scores_dev, uint64_t row_elems, uint32_t flags,
                                                 float *search_kernel_ms)
{
	if(!g || !fs){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_filter_scores_device: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::filter_scores_device(g, fs, scores_dev, row_elems, flags, search_kernel_ms, blocks, "kwage_search_filter_scores_device"));
}

extern "C" int kwage_search_filter_scores(kwage_group *g, kwage_filterset *fs, uint32_t *scores, uint64_t row_elems, uint32_t flags,
                                          float *search_kernel_ms)
{
	if(!g || !fs){ return kwage::fail(KWAGE_ERR_ARG, "kwage_search_filter_scores: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::filter_scores_host(g, fs, scores, row_elems, flags, search_kernel_ms, blocks));
}

extern "C" const char *kwage_search_filter_kernel(void) { return kwage::last_kernel; }

extern "C" int kwage_group_column_bits_device(kwage_group *g, void *out_dev)
{
	if(!g){ return kwage::fail(KWAGE_ERR_ARG, "kwage_group_column_bits_device: NULL argument"); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	return kwage::settle(g->ctx, kwage::column_bits_device(g, out_dev, blocks, "kwage_group_column_bits_device"));
}

extern "C" int kwage_group_column_bits(kwage_group *g, uint32_t *out)
{
	static const char *what = "kwage_group_column_bits";
	if(!g){ return kwage::fail(KWAGE_ERR_ARG, "%s: NULL argument", what); }
	const uint64_t span = g->next_byte*8;
	if(span && !out){ return kwage::fail(KWAGE_ERR_ARG, "%s: out is NULL", what); }
	kwage::PoolBlocks blocks(&g->ctx->batch_pool);
	uint32_t *d_out = nullptr;
	int rc = hipSetDevice(g->ctx->device) == hipSuccess ? KWAGE_OK : kwage::fail(KWAGE_ERR_DEVICE, "%s: hipSetDevice failed", what);
	if(!rc){ rc = blocks.take(std::max<uint64_t>(span, 4)*sizeof(uint32_t), &d_out); }
	if(!rc){ rc = kwage::column_bits_device(g, d_out, blocks, what); }
	if(!rc && span && hipMemcpy(out, d_out, (size_t)span*sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess){
		rc = kwage::fail(KWAGE_ERR_DEVICE, "%s: copying the counts back failed", what);
	}
	return kwage::settle(g->ctx, rc);
}
