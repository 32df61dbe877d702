// kwage_amd/csrc/export_plan.hpp -- the host-side planning of the export (export.hip, kwage_group_export_filters and its
// device and file forms): which columns may be exported and the runs their list folds into (the save's SaveRun table:
// destination = filter index, source = column), the rows of a staged chunk, the grid of a launch, and a host restatement
// of what the kernel stores -- filter f, dword j of a chunk -- built from the same save_word the kernel calls.  Plain
// functions of plain values: no device, no group -- tests/sanitize/export_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_EXPORT_PLAN_HPP
#define KWAGE_AMD_EXPORT_PLAN_HPP

#include "save_plan.hpp"

namespace kwage {

// The column list of an export folded into runs, in list order: filter i of the output is source column columns[i].
// Unlike a save's list it may name a column more than once (reading has no conflicts: the column is written twice).
// Refused (KWAGE_ERR_ARG, `runs` empty, the message names `who`): n == 0 or n > 2^32 - 1 (SaveRun counts in 32 bits), a
// column at or beyond the span, a pad or retired column of valid[] (the group's host valid mask, a bit per column, LSB
// first).
inline int plan_export(const char *who, const uint64_t *columns, uint64_t n, uint64_t span, const uint8_t *valid, std::vector<SaveRun> &runs)
{
	runs.clear();
	if(n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(n > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: %llu filters are more than one call exports", who, (unsigned long long)n); }
	for(uint64_t i = 0; i < n; ++i){
		const uint64_t c = columns[i];
		if(c >= span){ return fail(KWAGE_ERR_ARG, "%s: column %llu is at or beyond the span %llu", who, (unsigned long long)c, (unsigned long long)span); }
		if(!((valid[c/8] >> (c%8)) & 1)){ return fail(KWAGE_ERR_ARG, "%s: column %llu is a pad or retired column", who, (unsigned long long)c); }
	}
	for(uint64_t i = 0; i < n; ++i){
		if(!runs.empty() && columns[i] == runs.back().src_first + runs.back().len){ ++runs.back().len; }
		else{ runs.push_back(SaveRun{columns[i], (uint32_t)i, 1u}); }
	}
	return KWAGE_OK;
}

// A filter of a group of nrows = 2^L rows: max(1, nrows / 8) bytes.
inline uint64_t export_filter_bytes(uint64_t nrows) { return std::max<uint64_t>(1, nrows/8); }

// The chunks of the host and file forms.  A chunk is chunk_bytes bytes of every filter -- rows [r0, r0 + rows), rows a
// multiple of 8 (or all nrows < 8 rows of a filter of one byte) -- and the n pieces of a chunk fit `staging_bytes`, down
// to one byte of every filter per chunk; 0 means 64 MiB.  Chunks of 64 bytes and more are whole tiles' worth of rows
// (a multiple of 64 bytes = 512 rows), so that only a filter's last tile can be a partial one.  dev_stride: bytes between
// the pieces in the device staging block, a multiple of 4 -- and, from 256 bytes on, an ODD number of 256-byte units: a
// lane's 32 stores go to 32 consecutive filters at the same offset, and such pieces spread over the memory channels
// (as the insert stages its input).
struct ExportChunks { uint64_t filter_bytes, chunk_bytes, rows, chunks, dev_stride; };
inline ExportChunks plan_export_chunks(uint64_t staging_bytes, uint64_t n, uint64_t nrows)
{
	ExportChunks c;
	c.filter_bytes = export_filter_bytes(nrows);
	if(staging_bytes == 0){ staging_bytes = 64ull << 20; }
	c.chunk_bytes = std::min(std::max<uint64_t>(1, staging_bytes/std::max<uint64_t>(n, 1)), c.filter_bytes);
	if(c.chunk_bytes >= 64 && c.chunk_bytes < c.filter_bytes){ c.chunk_bytes = c.chunk_bytes/64*64; }
	c.rows = std::min(8*c.chunk_bytes, nrows);
	c.chunks = (c.filter_bytes + c.chunk_bytes - 1)/c.chunk_bytes;
	if(c.chunk_bytes < 256){ c.dev_stride = (c.chunk_bytes + 3)/4*4; }
	else{
		c.dev_stride = (c.chunk_bytes + 255)/256*256;
		if((c.dev_stride/256) % 2 == 0){ c.dev_stride += 256; }
	}
	return c;
}

// The grid of one launch: a workgroup per tile of tile_rows rows x tile_filters filters, row tiles first.  ok: the tiles
// fit one launch.
struct ExportGrid { uint64_t tiles_x, tiles_f; bool ok; };
inline ExportGrid export_grid(uint64_t chunk_rows, uint64_t n, uint64_t tile_rows, uint64_t tile_filters)
{
	ExportGrid g;
	g.tiles_x = (chunk_rows + tile_rows - 1)/tile_rows;
	g.tiles_f = (n + tile_filters - 1)/tile_filters;
	g.ok = g.tiles_x > 0 && g.tiles_f > 0 && g.tiles_f <= 0x7FFFFFFFull/g.tiles_x;
	return g;
}

// What the kernel stores as dword j of filter f (f < n) of a chunk of chunk_rows rows whose first row is row_base: bit b
// is row row_base + 32 j + b of the filter's source column, zero for rows beyond the chunk.  Restated with the kernel's
// own save_word over the 32 listed filters f belongs to; load(byte offset) returns the matrix's dword there.
template <typename LOAD>
inline uint32_t export_dword(LOAD &&load, const SaveRun *runs, uint32_t n_runs, uint32_t n, uint64_t row_base, uint64_t chunk_rows,
                             uint64_t stride, uint64_t matrix_bytes, uint32_t f, uint64_t j)
{
	const uint32_t d0 = f/32*32, d1 = (uint32_t)std::min<uint64_t>((uint64_t)d0 + 32, n);
	uint32_t v = 0;
	for(uint32_t b = 0; b < 32; ++b){
		const uint64_t r = 32*j + b;
		if(r >= chunk_rows){ break; }
		uint32_t k = save_find_run(runs, n_runs, d0);
		const uint32_t word = save_word(load, runs, &k, row_base + r, stride, matrix_bytes, d0, d1);
		v |= ((word >> (f - d0)) & 1u) << b;
	}
	return v;
}

}  // namespace kwage

#endif
