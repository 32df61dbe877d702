// kwage_amd/csrc/save.hip -- save: chosen columns of a group's RESIDENT matrix written as one raw `.db` file, packed
// densely on the device -- the missing half of the live insert (insert.hip); with a load behind it it also defragments
// what retire leaves (compact.hip does that in place).  No counterpart in the reference, whose only writer is build_db().
//
//   which columns, in what order   save_plan.hpp plan_save: the list folded into runs of consecutive columns
//   who writes what                save_kernels.hpp extract_columns_kernel: one thread per 16 bytes of an output row
//   the file                       db_writer.hpp: header, chunk loop with the CRC32 and the write on a host thread, metadata
//                                  index and records -- kwage_build_db's own, so the bytes are build_db()'s for the same filters
//
// Every refusal is found before out_path is touched; the file is written beside it and renamed at the end.  The group is
// only read.  Synchronous; runs on the context's first stream.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include <unistd.h>

#include "db_writer.hpp"
#include "engine_state.hpp"
#include "host.hpp"
#include "save_kernels.hpp"
#include "save_plan.hpp"
#include "save_records.hpp"

using namespace kwage;

namespace {

// extract_columns_kernel over one chunk of rows, queued on `stream`.
hipError_t launch_extract(const kwage_group *g, const SaveRun *d_runs, uint32_t n_runs, uint32_t n, uint64_t r0, uint64_t nr,
                          uint8_t *d_out, uint64_t out_slice, hipStream_t stream)
{
	const uint64_t total = nr*((out_slice + 15)/16);
	const dim3 grid((uint32_t)std::min<uint64_t>((total + 255)/256, 1u << 20)), block(256);
	const uint64_t matrix_bytes = g->nrows*g->stride;
	if(out_slice % 16 == 0){
		hipLaunchKernelGGL(extract_columns_kernel<16>, grid, block, 0, stream, g->d_bits, g->stride, matrix_bytes, d_runs, n_runs, n, r0, nr, d_out, out_slice);
	}
	else if(out_slice % 4 == 0){
		hipLaunchKernelGGL(extract_columns_kernel<4>, grid, block, 0, stream, g->d_bits, g->stride, matrix_bytes, d_runs, n_runs, n, r0, nr, d_out, out_slice);
	}
	else{
		hipLaunchKernelGGL(extract_columns_kernel<1>, grid, block, 0, stream, g->d_bits, g->stride, matrix_bytes, d_runs, n_runs, n, r0, nr, d_out, out_slice);
	}
	return hipGetLastError();
}

}  // namespace

extern "C" int kwage_group_save_db(kwage_group *g, const char *out_path, const kwage_save_column *cols, uint32_t n,
                                   uint64_t staging_bytes, kwage_save_stats *stats)
{
	const char *who = "kwage_group_save_db";
	if(!g || !out_path || !cols){ return fail(KWAGE_ERR_ARG, "%s: NULL argument", who); }
	if(n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(g->d_row_map){ return fail(KWAGE_ERR_ARG, "%s: a sparse group holds only some rows of its columns", who); }
	kwage_ctx *ctx = g->ctx;
	for(int i = 0; i < 2; ++i){ if(ctx->slot[i].busy){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); } }
	for(uint32_t i = 0; i < n; ++i){
		if(!cols[i].source_db && !cols[i].info){ return fail(KWAGE_ERR_ARG, "%s: entry %u has neither source_db nor info", who, i); }
	}
	std::vector<uint64_t> columns(n);
	for(uint32_t i = 0; i < n; ++i){ columns[i] = cols[i].column; }
	std::vector<SaveRun> runs;
	int rc = plan_save(columns.data(), n, g->next_byte*8, g->h_valid.data(), runs);
	if(rc){ return rc; }
	const SaveChunks ch = plan_chunks(staging_bytes, n, g->nrows);
	if(ch.chunks > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: staging_bytes %llu cuts the file into too many chunks", who, (unsigned long long)staging_bytes); }
	std::vector<uint64_t> rec_len;
	std::vector<unsigned char> recs;
	if((rc = collect_records(who, cols, n, rec_len, recs))){ return rc; }
	if((rc = set_device(ctx))){ return rc; }

	// the device side: the run table and one chunk of output
	DevBuf d_runs, d_out;
	if((rc = d_runs.reserve(runs.size()*sizeof(SaveRun))) || (rc = d_out.reserve(ch.rows*ch.out_slice))){ d_runs.release(); return rc; }
	auto release = [&]() { d_runs.release(); d_out.release(); };
	hipError_t e = hipMemcpyAsync(d_runs.p, runs.data(), runs.size()*sizeof(SaveRun), hipMemcpyHostToDevice, ctx->stream);
	if(e == hipSuccess){ e = hipStreamSynchronize(ctx->stream); }
	if(e != hipSuccess){ release(); return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }

	// the file, under a temporary name beside out_path
	const std::string tmp = std::string(out_path) + ".saving." + std::to_string((long long)getpid());
	FILE *fout = fopen(tmp.c_str(), "wb");
	if(!fout){ release(); return fail(KWAGE_ERR_IO, "%s: Unable to open %s for writing", who, tmp.c_str()); }
	unsigned char hdr[DB_HEADER_BYTES];
	db_header_placeholder(hdr, g->params, n);
	bool ok = fwrite(hdr, 1, sizeof(hdr), fout) == sizeof(hdr);
	uint32_t crc = 0, n_chunk = 0;
	double kernel_ms = 0;
	auto extract_chunk = [&](uint64_t r0, uint64_t nr, hipEvent_t ev0, hipEvent_t ev1) -> hipError_t {
		(void)hipEventRecord(ev0, ctx->stream);
		const hipError_t le = launch_extract(g, (const SaveRun*)d_runs.p, (uint32_t)runs.size(), n, r0, nr, (uint8_t*)d_out.p, ch.out_slice, ctx->stream);
		(void)hipEventRecord(ev1, ctx->stream);
		return le;
	};
	e = write_db_body(fout, ctx->stream, g->nrows, ch.rows, ch.out_slice, d_out.p, extract_chunk, &crc, &ok, &kernel_ms, &n_chunk);
	release();
	uint64_t db_bytes = 0;
	if(e == hipSuccess){ ok = write_db_tail(fout, hdr, crc, DB_HEADER_BYTES + g->nrows*ch.out_slice, rec_len, recs, &db_bytes) && ok; }
	ok = (fclose(fout) == 0) && ok;
	if(e != hipSuccess){ (void)remove(tmp.c_str()); return fail(KWAGE_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e)); }
	if(ok && rename(tmp.c_str(), out_path) != 0){ ok = false; }
	if(!ok){ (void)remove(tmp.c_str()); return fail(KWAGE_ERR_IO, "%s: Error writing database file %s", who, out_path); }
	if(stats){
		stats->db_bytes = db_bytes;
		stats->runs = runs.size();
		stats->chunks = n_chunk;
		stats->extract_kernel_ms = (float)kernel_ms;
	}
	return KWAGE_OK;
}
