// kwage_amd/csrc/export.hip -- export: listed columns of a group's RESIDENT matrix handed back as what they were made from,
// whole Bloom filters (2^L bits each, filter-major, LSB first: the payload of a `.bloom` file), transposed on the device
// -- the inverse of the live insert (insert.hip).  The reference only has dump_bloom / dump_db to look at such objects.
//
//   which columns, in what order   export_plan.hpp plan_export: the list folded into the save's runs of consecutive columns
//   who writes what                export_kernels.hpp export_filters_kernel: the insert's tile run backwards, one thread per
//                                  (filter, dword of rows)
//   the three forms                host memory (chunks of rows staged through the context's load buffer, one strided copy
//                                  per chunk), device memory in place, and `.bloom` files (records as the save takes them:
//                                  save_records.hpp; CRC32 chunk by chunk; temporary names, renamed once all are complete)
//
// Every refusal is found before a byte of the caller's memory or of any file is written.  The group is only read.
// Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include <unistd.h>
#include <zlib.h>

#include "engine_state.hpp"
#include "export_kernels.hpp"
#include "export_plan.hpp"
#include "save_records.hpp"

using namespace kwage;

// host.cpp
namespace kwage { void bloom_file_head(const kwage_params *params, uint32_t crc, std::vector<unsigned char> &head); }

namespace {

using ExportTile = TransposeTile<16, 8>;      // the insert's shape: 512 rows x 32 words (1024 filters; 64-byte runs of a filter per 16 lanes)

const uint32_t BLOOM_CRC_AT = 17;             // the CRC32 of a `.bloom` file: behind the magic and the four BloomParam words
const uint32_t FILES_OPEN = 256;              // `.bloom` files written side by side: the file form goes through its list in such batches

struct Events {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	~Events() { if(ev0){ (void)hipEventDestroy(ev0); } if(ev1){ (void)hipEventDestroy(ev1); } }
};

// A block of the context's pool, handed back when the call ends.
struct PoolBlock {
	DevPool *pool;
	void *p = nullptr;
	uint64_t cap = 0;
	explicit PoolBlock(DevPool *pl) : pool(pl) {}
	~PoolBlock() { if(p){ pool->give(p, cap); } }
	PoolBlock(const PoolBlock&) = delete;
	PoolBlock &operator=(const PoolBlock&) = delete;
};

// export_filters_kernel over one chunk of rows, queued on `stream`.
hipError_t launch_export(const kwage_group *g, const SaveRun *d_runs, uint32_t n_runs, uint32_t n, uint64_t r0, uint64_t nr,
                         uint8_t *d_out, uint64_t out_stride, hipStream_t stream)
{
	using T = ExportTile;
	const ExportGrid grid = export_grid(nr, n, T::ROWS, T::FILTERS);
	if(!grid.ok){ return hipErrorInvalidValue; }
	hipLaunchKernelGGL((export_filters_kernel<T::ROWS/32, T::WAVES>), dim3((uint32_t)(grid.tiles_x*grid.tiles_f)), dim3(T::WAVES*64), 0, stream,
	                   g->d_bits, g->stride, g->nrows*g->stride, d_runs, n_runs, n, r0, nr, d_out, out_stride, (uint32_t)grid.tiles_x);
	return hipGetLastError();
}

// What every form checks first, and the plan.
int export_prepare(const kwage_group *g, const uint64_t *columns, uint32_t n, const char *who, std::vector<SaveRun> &runs)
{
	if(n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group holds only some rows of its columns", who); }
	for(int i = 0; i < 2; ++i){ if(g->ctx->slot[i].busy){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); } }
	return plan_export(who, columns, n, g->next_byte*8, g->h_valid.data(), runs);
}

// The run table on the device, in a block of the context's pool.
int upload_runs(kwage_ctx *ctx, const std::vector<SaveRun> &runs, PoolBlock &d_runs)
{
	HIP_TRY(ctx->batch_pool.take(runs.size()*sizeof(SaveRun), &d_runs.p, &d_runs.cap));
	HIP_TRY(hipMemcpyAsync(d_runs.p, runs.data(), runs.size()*sizeof(SaveRun), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return KWAGE_OK;
}

// The host and file forms' work for one planned list: chunk after chunk of rows, the kernel into the context's load
// staging buffer, then copy(first byte of the chunk within a filter, its bytes per filter, the staged pieces, their
// stride) queues what takes the chunk off the device, and done(first byte, bytes) runs once it has arrived (false: stop,
// the caller knows why).  *kernel_ms grows by the events' durations.
template <typename COPY, typename DONE>
int export_staged(kwage_group *g, const std::vector<SaveRun> &runs, uint32_t n, uint64_t staging_bytes, bool timing, double *kernel_ms,
                  COPY &&copy, DONE &&done)
{
	kwage_ctx *ctx = g->ctx;
	const ExportChunks ch = plan_export_chunks(staging_bytes, n, g->nrows);
	int rc;
	if((rc = ctx->load_dev[0].reserve(ch.dev_stride*n))){ return rc; }
	PoolBlock d_runs(&ctx->batch_pool);
	if((rc = upload_runs(ctx, runs, d_runs))){ return rc; }
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	uint8_t *d_stage = (uint8_t*)ctx->load_dev[0].p;
	for(uint64_t b0 = 0; b0 < ch.filter_bytes; b0 += ch.chunk_bytes){
		const uint64_t nb = std::min(ch.chunk_bytes, ch.filter_bytes - b0);
		const uint64_t r0 = 8*b0, nr = std::min(8*nb, g->nrows - r0);
		if(timing){ HIP_TRY(hipEventRecord(ev.ev0, ctx->stream)); }
		HIP_TRY(launch_export(g, (const SaveRun*)d_runs.p, (uint32_t)runs.size(), n, r0, nr, d_stage, ch.dev_stride, ctx->stream));
		if(timing){ HIP_TRY(hipEventRecord(ev.ev1, ctx->stream)); }
		HIP_TRY(copy(b0, nb, d_stage, ch.dev_stride));
		HIP_TRY(hipStreamSynchronize(ctx->stream));          // the staging block is the next chunk's
		if(timing){ float ms = 0; (void)hipEventElapsedTime(&ms, ev.ev0, ev.ev1); *kernel_ms += ms; }
		if(!done(b0, nb)){ return KWAGE_ERR_IO; }
	}
	return KWAGE_OK;
}

}  // namespace

extern "C" int kwage_group_export_filters(kwage_group *g, const uint64_t *columns, uint32_t n, void *bits,
                                          uint64_t filter_stride_bytes, uint64_t staging_bytes, uint32_t flags, float *export_kernel_ms)
{
	const char *who = "kwage_group_export_filters";
	if(!g || !columns || !bits){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	const uint64_t filter_bytes = export_filter_bytes(g->nrows);
	if(n > 1 && filter_stride_bytes < filter_bytes){ return fail(KWAGE_ERR_ARG, "%s: filter_stride_bytes is smaller than a filter", who); }
	std::vector<SaveRun> runs;
	int rc = export_prepare(g, columns, n, who, runs);
	if(rc){ return rc; }
	if((rc = set_device(g->ctx))){ return rc; }
	kwage_ctx *ctx = g->ctx;
	double ms = 0;
	// n pieces of nb bytes leave the device in one copy, to filter_stride_bytes apart
	auto copy = [&](uint64_t b0, uint64_t nb, const uint8_t *d_stage, uint64_t dev_stride) {
		return hipMemcpy2DAsync((uint8_t*)bits + b0, n > 1 ? filter_stride_bytes : nb, d_stage, dev_stride, nb, n, hipMemcpyDeviceToHost, ctx->stream);
	};
	auto done = [](uint64_t, uint64_t) { return true; };
	if((rc = export_staged(g, runs, n, staging_bytes, (flags & KWAGE_SEARCH_TIMING) != 0, &ms, copy, done))){ return rc; }
	if(export_kernel_ms){ *export_kernel_ms = (float)ms; }
	return KWAGE_OK;
}

extern "C" int kwage_group_export_filters_device(kwage_group *g, const uint64_t *columns, uint32_t n, void *bits_dev,
                                                 uint64_t filter_stride_bytes, uint32_t flags, float *export_kernel_ms)
{
	const char *who = "kwage_group_export_filters_device";
	if(!g || !columns || !bits_dev){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	const uint64_t filter_bytes = export_filter_bytes(g->nrows);
	if((((uintptr_t)bits_dev) & 3) || (filter_stride_bytes & 3)){ return fail(KWAGE_ERR_ARG, "%s: pointer and stride must be multiples of 4", who); }
	if(n > 1 && filter_stride_bytes < filter_bytes){ return fail(KWAGE_ERR_ARG, "%s: filter_stride_bytes is smaller than a filter", who); }
	std::vector<SaveRun> runs;
	int rc = export_prepare(g, columns, n, who, runs);
	if(rc){ return rc; }
	if((rc = set_device(g->ctx))){ return rc; }
	kwage_ctx *ctx = g->ctx;
	PoolBlock d_runs(&ctx->batch_pool);
	if((rc = upload_runs(ctx, runs, d_runs))){ return rc; }
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	Events ev;
	if(timing){ HIP_TRY(hipEventCreate(&ev.ev0)); HIP_TRY(hipEventCreate(&ev.ev1)); }
	// (filters shorter than a dword are written byte by byte: nothing beyond a filter's own bytes is touched)
	if(timing){ HIP_TRY(hipEventRecord(ev.ev0, ctx->stream)); }
	HIP_TRY(launch_export(g, (const SaveRun*)d_runs.p, (uint32_t)runs.size(), n, 0, g->nrows, (uint8_t*)bits_dev,
	                      n > 1 ? filter_stride_bytes : (filter_bytes + 3)/4*4, ctx->stream));
	if(timing){ HIP_TRY(hipEventRecord(ev.ev1, ctx->stream)); }
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	float ms = 0;
	if(timing){ (void)hipEventElapsedTime(&ms, ev.ev0, ev.ev1); }
	if(export_kernel_ms){ *export_kernel_ms = ms; }
	return KWAGE_OK;
}

extern "C" int kwage_group_export_bloom_files(kwage_group *g, const kwage_save_column *cols, const char *const *out_paths, uint32_t n,
                                              uint64_t staging_bytes, uint32_t flags, float *export_kernel_ms)
{
	const char *who = "kwage_group_export_bloom_files";
	if(!g || !cols || !out_paths){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	for(uint32_t i = 0; i < n; ++i){
		if(!cols[i].source_db && !cols[i].info){ return fail(KWAGE_ERR_ARG, "%s: entry %u has neither source_db nor info", who, i); }
		if(!out_paths[i]){ return fail(KWAGE_ERR_ARG, "%s: entry %u has no path", who, i); }
	}
	std::vector<uint64_t> columns(n);
	for(uint32_t i = 0; i < n; ++i){ columns[i] = cols[i].column; }
	std::vector<SaveRun> runs;
	int rc = export_prepare(g, columns.data(), n, who, runs);
	if(rc){ return rc; }
	std::vector<uint64_t> rec_len;
	std::vector<unsigned char> recs;
	if((rc = collect_records(who, cols, n, rec_len, recs))){ return rc; }
	if((rc = set_device(g->ctx))){ return rc; }
	kwage_ctx *ctx = g->ctx;

	// every file under a temporary name beside its destination; whatever fails, none of them stays
	const std::string suffix = ".exporting." + std::to_string((long long)getpid());
	std::vector<std::string> tmp;          // the temporary files made so far
	auto drop_all = [&]() { for(const std::string &t : tmp){ (void)remove(t.c_str()); } };
	double ms = 0;
	const bool timing = (flags & KWAGE_SEARCH_TIMING) != 0;
	uint64_t rec_at = 0;
	for(uint32_t i0 = 0; i0 < n; i0 += FILES_OPEN){
		const uint32_t m = std::min(FILES_OPEN, n - i0);
		if((rc = plan_export(who, columns.data() + i0, m, g->next_byte*8, g->h_valid.data(), runs))){ drop_all(); return rc; }
		std::vector<FILE*> files(m, nullptr);
		std::vector<uint32_t> crc(m, (uint32_t)crc32_z(0L, Z_NULL, 0));
		auto close_all = [&]() { bool ok = true; for(FILE *&f : files){ if(f){ ok = (fclose(f) == 0) && ok; f = nullptr; } } return ok; };
		bool ok = true;
		for(uint32_t i = 0; i < m && ok; ++i){
			const std::string t = std::string(out_paths[i0 + i]) + suffix;
			files[i] = fopen(t.c_str(), "wb");
			if(!files[i]){ close_all(); drop_all(); return fail(KWAGE_ERR_IO, "%s: Unable to open %s for writing", who, t.c_str()); }
			tmp.push_back(t);
			std::vector<unsigned char> head;
			bloom_file_head(&g->params, 0, head);          // (the CRC32 follows the bits)
			ok = fwrite(head.data(), 1, head.size(), files[i]) == head.size() &&
			     fwrite(recs.data() + rec_at, 1, rec_len[i0 + i], files[i]) == rec_len[i0 + i];
			rec_at += rec_len[i0 + i];
		}
		if(ok){
			// a chunk's n pieces land densely in the context's pinned load buffer; each filter's CRC32 and file take their piece
			const ExportChunks ch = plan_export_chunks(staging_bytes, m, g->nrows);
			if((rc = ctx->load_pin[0].reserve(ch.chunk_bytes*m))){ close_all(); drop_all(); return rc; }
			uint8_t *h = (uint8_t*)ctx->load_pin[0].p;
			auto copy = [&](uint64_t, uint64_t nb, const uint8_t *d_stage, uint64_t dev_stride) {
				return hipMemcpy2DAsync(h, nb, d_stage, dev_stride, nb, m, hipMemcpyDeviceToHost, ctx->stream);
			};
			auto done = [&](uint64_t, uint64_t nb) {
				for(uint32_t i = 0; i < m; ++i){
					crc[i] = (uint32_t)crc32_z(crc[i], h + (uint64_t)i*nb, nb);
					if(fwrite(h + (uint64_t)i*nb, 1, nb, files[i]) != nb){ return false; }
				}
				return true;
			};
			rc = export_staged(g, runs, m, staging_bytes, timing, &ms, copy, done);
			if(rc == KWAGE_ERR_IO){ ok = false; rc = KWAGE_OK; }
			if(rc){ close_all(); drop_all(); return rc; }
		}
		for(uint32_t i = 0; i < m && ok; ++i){
			unsigned char c[4];
			for(int k = 0; k < 4; ++k){ c[k] = (unsigned char)(crc[i] >> (8*k)); }
			ok = fseek(files[i], BLOOM_CRC_AT, SEEK_SET) == 0 && fwrite(c, 1, 4, files[i]) == 4;
		}
		ok = close_all() && ok;
		if(!ok){ drop_all(); return fail(KWAGE_ERR_IO, "%s: Error writing Bloom filter files", who); }
	}
	for(uint32_t i = 0; i < n; ++i){
		if(rename(tmp[i].c_str(), out_paths[i]) != 0){
			for(uint32_t k = i; k < n; ++k){ (void)remove(tmp[k].c_str()); }
			return fail(KWAGE_ERR_IO, "%s: Unable to rename %s to %s", who, tmp[i].c_str(), out_paths[i]);
		}
	}
	if(export_kernel_ms){ *export_kernel_ms = (float)ms; }
	return KWAGE_OK;
}
