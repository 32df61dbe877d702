// kwage_amd/csrc/insert.hip -- live insert: whole Bloom filters become new columns of a group's RESIDENT matrix, before or
// after kwage_group_finalize, without touching the columns already there; and the companion, retiring columns.  No
// counterpart in the reference, whose databases are written once (build_db.cpp) and read from disk.
//
//   where the columns go       insert_plan.hpp plan_insert: inserts pack densely at bit granularity behind each other; the
//                              first one after any other block starts on a 16-byte boundary of the row like every block
//   who writes what            insert_kernels.hpp insert_filters_kernel: the builder's tile (transpose_tile.hpp) written
//                              into the strided matrix at a bit offset; one thread per (row, 32-column word), no atomics
//   the state a call leaves    h_valid / the changed bytes of d_valid, next_byte, num_columns, the open tail, and -- for a
//                              finalized group -- density / density_max re-sampled with finalize's probe (loader.hip)
//
// Every refusal is found before anything is written; the calls are synchronous and run on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bloom_files.hpp"
#include "engine_state.hpp"
#include "insert_kernels.hpp"
#include "insert_plan.hpp"

using namespace kwage;

// loader.hip
namespace kwage { void group_probe_density(kwage_group *g); }
// (defined below; copy.hip calls it too)
namespace kwage { int commit_insert(kwage_group *g, uint64_t first, uint64_t n); }

namespace {

using InsertTile = TransposeTile<16, 8>;      // the builder's default shape: 512 rows x 32 words (128-byte row segments)

int refuse_pending(const kwage_ctx *ctx, const char *who)
{
	for(int i = 0; i < 2; ++i){ if(ctx->slot[i].busy){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); } }
	return KWAGE_OK;
}

// insert_filters_kernel over one chunk of rows, queued on `stream`.
hipError_t launch_insert(const uint8_t *d_in, uint64_t in_stride, uint32_t n, uint64_t chunk_rows, kwage_group *g, uint64_t row_base,
                         const InsertSpan &sp, hipStream_t stream)
{
	using T = InsertTile;
	const uint64_t tiles_x = (chunk_rows + T::ROWS - 1)/T::ROWS;
	const uint64_t tiles_w = (sp.word_last - sp.word_base)/T::PITCH + 1;
	if(tiles_x*tiles_w > 0x7FFFFFFFull){ return hipErrorInvalidValue; }
	hipLaunchKernelGGL((insert_filters_kernel<T::ROWS/32, T::WAVES>), dim3((uint32_t)(tiles_x*tiles_w)), dim3(T::WAVES*64), 0, stream,
	                   d_in, in_stride, n, chunk_rows, g->d_bits, g->stride, row_base,
	                   sp.word_base, sp.word_first, sp.word_last, sp.keep_bits, sp.shift, (uint32_t)tiles_x);
	return hipGetLastError();
}

}  // namespace

// The columns first .. first + n - 1 are in the matrix: the group's state follows.  (Shared with the copy between groups,
// copy.hip, whose columns arrive exactly as an insert's do.)
int kwage::commit_insert(kwage_group *g, uint64_t first, uint64_t n)
{
	kwage_ctx *ctx = g->ctx;
	for(uint64_t c = first; c < first + n; ++c){ g->h_valid[c/8] |= (uint8_t)(1u << (c%8)); }
	g->tail_column = first + n;
	g->tail_open = true;
	g->next_byte = (first + n + 7)/8;
	g->num_columns += n;
	const uint64_t b0 = first/8;
	HIP_TRY(hipMemcpyAsync(g->d_valid + b0, g->h_valid.data() + b0, g->next_byte - b0, hipMemcpyHostToDevice, ctx->stream));
	if(g->finalized){ group_probe_density(g); }      // (before finalize, finalize samples it)
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return KWAGE_OK;
}

namespace {

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

// The host form's work, for filters at base + i*stride (ptrs == NULL) or at ptrs[i]: chunks of rows staged through the
// context's load staging buffers, the kernel on each chunk.
int insert_from_host(kwage_group *g, const uint8_t *base, uint64_t filter_stride, const uint8_t *const *ptrs, uint32_t n,
                     uint32_t flags, uint64_t first, float *kernel_ms)
{
	kwage_ctx *ctx = g->ctx;
	const uint32_t lg = g->params.log_2_filter_len;
	const uint64_t nrows = g->nrows;
	const InsertSpan sp = insert_span(first, n);
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	double ms_total = 0;
	int rc;
	auto filter = [&](uint32_t i) { return ptrs ? ptrs[i] : base + (uint64_t)i*filter_stride; };

	if(lg < 5){
		// filters shorter than a dword: one aligned dword per filter, put together on the host (bits beyond 2^L cleared)
		const uint32_t mask = (1u << nrows) - 1;
		if((rc = ctx->load_pin[0].reserve(4ull*n)) || (rc = ctx->load_dev[0].reserve(4ull*n))){ return rc; }
		uint32_t *h = (uint32_t*)ctx->load_pin[0].p;
		for(uint32_t i = 0; i < n; ++i){
			const uint8_t *f = filter(i);
			uint32_t v = f[0];
			if(lg == 4){ v |= (uint32_t)f[1] << 8; }
			h[i] = v & mask;
		}
		HIP_TRY(hipMemcpyAsync(ctx->load_dev[0].p, h, 4ull*n, hipMemcpyHostToDevice, ctx->stream));
		if(timing){ HIP_TRY(hipEventRecord(ev.ev0, ctx->stream)); }
		HIP_TRY(launch_insert((const uint8_t*)ctx->load_dev[0].p, 4, n, nrows, g, 0, sp, ctx->stream));
		if(timing){ HIP_TRY(hipEventRecord(ev.ev1, ctx->stream)); }
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if(timing){ float ms = 0; (void)hipEventElapsedTime(&ms, ev.ev0, ev.ev1); ms_total += ms; }
	}
	else{
		// chunk rows: the n pieces of a chunk stay within 64 MiB of staging
		uint64_t chunk_rows = nrows;
		while(chunk_rows > 1024 && chunk_rows/8*n > (64ull << 20)){ chunk_rows /= 2; }
		// a lane's 32 loads go to 32 consecutive filters at the same offset: pieces an ODD number of 256-byte units apart
		// spread them over the memory channels (builder.hip, profiles/r04_builder_transpose.txt)
		uint64_t in_stride = (chunk_rows/8 + 255)/256*256;
		if((in_stride/256) % 2 == 0){ in_stride += 256; }
		if((rc = ctx->load_dev[0].reserve(in_stride*n))){ return rc; }
		if(ptrs && (rc = ctx->load_pin[0].reserve(in_stride*n))){ return rc; }
		for(uint64_t r0 = 0; r0 < nrows; r0 += chunk_rows){
			const uint64_t nr = std::min(chunk_rows, nrows - r0), nb = nr/8;
			if(ptrs){
				// filters that lie apart (mapped `.bloom` payloads): this chunk of each into the pinned block, one copy
				for(uint32_t i = 0; i < n; ++i){ memcpy((uint8_t*)ctx->load_pin[0].p + (uint64_t)i*in_stride, ptrs[i] + r0/8, nb); }
				HIP_TRY(hipMemcpyAsync(ctx->load_dev[0].p, ctx->load_pin[0].p, in_stride*(n - 1) + nb, hipMemcpyHostToDevice, ctx->stream));
			}
			else{
				// n pieces of nb bytes, filter_stride_bytes apart, in one copy
				HIP_TRY(hipMemcpy2DAsync(ctx->load_dev[0].p, in_stride, base + r0/8, n > 1 ? filter_stride : nb, nb, n, hipMemcpyHostToDevice, ctx->stream));
			}
			if(timing){ HIP_TRY(hipEventRecord(ev.ev0, ctx->stream)); }
			HIP_TRY(launch_insert((const uint8_t*)ctx->load_dev[0].p, in_stride, n, nr, g, r0, sp, ctx->stream));
			if(timing){ HIP_TRY(hipEventRecord(ev.ev1, ctx->stream)); }
			HIP_TRY(hipStreamSynchronize(ctx->stream));      // the staging blocks are the next chunk's
			if(timing){ float ms = 0; (void)hipEventElapsedTime(&ms, ev.ev0, ev.ev1); ms_total += ms; }
		}
	}
	if(kernel_ms){ *kernel_ms = (float)ms_total; }
	return KWAGE_OK;
}

// What every form checks first; *first = where the call's columns go.
int insert_prepare(kwage_group *g, uint32_t n, const char *who, uint64_t *first)
{
	if(n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group takes no inserts", who); }
	int rc = refuse_pending(g->ctx, who);
	if(rc){ return rc; }
	if((rc = plan_insert(g->next_byte, g->tail_open, g->tail_column, g->stride, n, first))){ return rc; }
	return set_device(g->ctx);
}

}  // namespace

extern "C" int kwage_group_insert_filters(kwage_group *g, const void *bits, uint64_t filter_stride_bytes, uint32_t n,
                                          uint32_t flags, uint64_t *first_column, float *insert_kernel_ms)
{
	if(!g || !bits || !first_column){ return fail(KWAGE_ERR_ARG, "kwage_group_insert_filters: NULL argument"); }
	const uint64_t filter_bytes = ((1ull << g->params.log_2_filter_len) + 7)/8;
	if(n > 1 && filter_stride_bytes < filter_bytes){ return fail(KWAGE_ERR_ARG, "kwage_group_insert_filters: filter_stride_bytes is smaller than a filter"); }
	uint64_t first = 0;
	int rc = insert_prepare(g, n, "kwage_group_insert_filters", &first);
	if(rc){ return rc; }
	if(insert_kernel_ms){ *insert_kernel_ms = 0; }
	if((rc = insert_from_host(g, (const uint8_t*)bits, filter_stride_bytes, nullptr, n, flags, first, insert_kernel_ms))){ return rc; }
	if((rc = commit_insert(g, first, n))){ return rc; }
	*first_column = first;
	return KWAGE_OK;
}

extern "C" int kwage_group_insert_filters_device(kwage_group *g, const void *bits_dev, uint64_t filter_stride_bytes, uint32_t n,
                                                 uint32_t flags, uint64_t *first_column, float *insert_kernel_ms)
{
	const char *who = "kwage_group_insert_filters_device";
	if(!g || !bits_dev || !first_column){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	const uint64_t filter_bytes = ((1ull << g->params.log_2_filter_len) + 7)/8;
	if((((uintptr_t)bits_dev) & 3) || (filter_stride_bytes & 3)){ return fail(KWAGE_ERR_ARG, "%s: pointer and stride must be multiples of 4", who); }
	if(n > 1 && filter_stride_bytes < filter_bytes){ return fail(KWAGE_ERR_ARG, "%s: filter_stride_bytes is smaller than a filter", who); }
	uint64_t first = 0;
	int rc = insert_prepare(g, n, who, &first);
	if(rc){ return rc; }
	kwage_ctx *ctx = g->ctx;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	if(insert_kernel_ms){ *insert_kernel_ms = 0; }
	// (filters shorter than a dword are read byte by byte: nothing beyond a filter's own bytes is touched)
	if(timing){ HIP_TRY(hipEventRecord(ev.ev0, ctx->stream)); }
	HIP_TRY(launch_insert((const uint8_t*)bits_dev, n > 1 ? filter_stride_bytes : (filter_bytes + 3)/4*4, n, g->nrows, g, 0, insert_span(first, n), ctx->stream));
	if(timing){ HIP_TRY(hipEventRecord(ev.ev1, ctx->stream)); }
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(timing && insert_kernel_ms){ (void)hipEventElapsedTime(insert_kernel_ms, ev.ev0, ev.ev1); }
	if((rc = commit_insert(g, first, n))){ return rc; }
	*first_column = first;
	return KWAGE_OK;
}

extern "C" int kwage_group_insert_bloom_files(kwage_group *g, const char *const *paths, uint32_t n, uint32_t flags,
                                              uint64_t *first_column, float *insert_kernel_ms)
{
	const char *who = "kwage_group_insert_bloom_files";
	if(!g || !paths || !first_column){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	uint64_t first = 0;
	int rc = insert_prepare(g, n, who, &first);
	if(rc){ return rc; }
	// all n files are opened and checked (parameters, CRC32) before the first column is written
	std::vector<BloomFile> files;
	if((rc = open_bloom_files(who, paths, n, &g->params, files))){ return rc; }
	std::vector<const uint8_t*> ptrs(n);
	for(uint32_t i = 0; i < n; ++i){ ptrs[i] = files[i].map + files[i].bits_off; }
	if(insert_kernel_ms){ *insert_kernel_ms = 0; }
	rc = insert_from_host(g, nullptr, 0, ptrs.data(), n, flags, first, insert_kernel_ms);
	for(auto &f : files){ f.close_file(); }
	if(rc){ return rc; }
	if((rc = commit_insert(g, first, n))){ return rc; }
	*first_column = first;
	return KWAGE_OK;
}

extern "C" int kwage_group_retire_columns(kwage_group *g, const uint64_t *columns, uint64_t n)
{
	const char *who = "kwage_group_retire_columns";
	if(!g || (n && !columns)){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	if(n == 0){ return KWAGE_OK; }
	kwage_ctx *ctx = g->ctx;
	int rc = refuse_pending(ctx, who);
	if(rc){ return rc; }
	std::vector<RetirePair> pairs;
	uint64_t distinct = 0;
	if((rc = plan_retire(g->h_valid.data(), g->next_byte*8, columns, n, pairs, &distinct))){ return rc; }
	if((rc = set_device(ctx))){ return rc; }
	DevBuf dp;
	if((rc = dp.reserve(pairs.size()*sizeof(RetirePair)))){ return rc; }
	hipError_t e = hipMemcpyAsync(dp.p, pairs.data(), pairs.size()*sizeof(RetirePair), hipMemcpyHostToDevice, ctx->stream);
	if(e == hipSuccess){
		const uint64_t work = g->nrows*pairs.size();
		hipLaunchKernelGGL(retire_columns_kernel, dim3((uint32_t)std::min<uint64_t>((work + 255)/256, 256*16)), dim3(256), 0, ctx->stream,
		                   g->d_bits, g->stride, g->nrows, (const RetirePair*)dp.p, (uint64_t)pairs.size());
		e = hipGetLastError();
	}
	if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
	dp.release();
	if(e != hipSuccess){ return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
	// the columns are pad columns from here on
	uint64_t b0 = g->stride, b1 = 0;
	for(const RetirePair &p : pairs){
		for(uint32_t k = 0; k < 4; ++k){ g->h_valid[4*p.word + k] &= (uint8_t)~(p.mask >> (8*k)); }
		b0 = std::min(b0, 4*p.word);
		b1 = std::max(b1, 4*p.word + 4);
	}
	g->num_columns -= distinct;
	HIP_TRY(hipMemcpyAsync(g->d_valid + b0, g->h_valid.data() + b0, b1 - b0, hipMemcpyHostToDevice, ctx->stream));
	if(g->finalized){ group_probe_density(g); }
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return KWAGE_OK;
}
