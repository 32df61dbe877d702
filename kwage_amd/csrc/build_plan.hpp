// kwage_amd/csrc/build_plan.hpp -- the host-side planning of the builder (builder.hip, kwage_build_db) and of the re-pack
// (kwage_repack_db): the rows of a chunk, the chunks, and for the builder how far apart the filters lie in the device's
// input block.  Plain functions of plain values: no device, no file -- tests/sanitize/build_plan_sanitize.cpp drives
// them under the sanitizers at sizes no GPU test can afford.
#ifndef KWAGE_AMD_BUILD_PLAN_HPP
#define KWAGE_AMD_BUILD_PLAN_HPP

#include <algorithm>
#include <cstdint>

namespace kwage {

// What both entry points call "budget" when none is given (0): input and output of a chunk stay at or below it.
static constexpr uint64_t BUILD_DEFAULT_BUDGET_BYTES = 256ull << 20;
// The builder never takes fewer rows per chunk, whatever the budget (or the whole filter where that is shorter).
static constexpr uint64_t BUILD_MIN_CHUNK_ROWS = 1024;

// kwage_build_db: n filters of filter_len = 2^L bits each -> a slice block of filter_len rows of ceil(n / 8) bytes.
//   chunk_rows: filter_len halved until the chunk's input (n x chunk_rows / 8 bytes) and its output (chunk_rows x slice
//               bytes; double-buffered on the host, db_writer.hpp write_db_body) both fit the budget, never below
//               BUILD_MIN_CHUNK_ROWS: a power of two that divides filter_len.
//   in_stride:  bytes between two filters in the device's input block.  A lane's 32 loads go to 32 consecutive filters
//               at the same offset: with a power-of-two stride they all fall on the same few memory channels (3.87 TB/s
//               in + out; a stride of an ODD number of 256-byte units: 4.43-4.50, profiles/r04_builder_transpose.txt).
//               pad_bytes >= 0 (KWAGE_BUILD_PAD): the chunk's bytes rounded up to 4, plus pad_bytes rounded down to 4,
//               instead -- never below the chunk itself.
//   chunks:     filter_len / chunk_rows.
struct BuildChunks { uint64_t chunk_rows, in_stride, chunks; };
inline BuildChunks plan_build_chunks(uint64_t budget_bytes, uint64_t n, uint64_t filter_len, long long pad_bytes = -1)
{
	if(budget_bytes == 0){ budget_bytes = BUILD_DEFAULT_BUDGET_BYTES; }
	const uint64_t slice_size = (n + 7)/8;
	BuildChunks c;
	c.chunk_rows = filter_len;
	while(c.chunk_rows > BUILD_MIN_CHUNK_ROWS && (c.chunk_rows/8*n > budget_bytes || c.chunk_rows*slice_size > budget_bytes)){ c.chunk_rows /= 2; }
	const uint64_t chunk_bytes = (c.chunk_rows + 7)/8;
	c.in_stride = (chunk_bytes + 255)/256*256;
	if((c.in_stride/256) % 2 == 0){ c.in_stride += 256; }
	if(pad_bytes >= 0){ c.in_stride = (chunk_bytes + 3)/4*4 + (uint64_t)pad_bytes/4*4; }
	c.chunks = (filter_len + c.chunk_rows - 1)/c.chunk_rows;
	return c;
}

// kwage_repack_db: nrows rows; a chunk's destination rows (dst_words dwords each on the device) and the widest source's
// rows (max_width bytes each) both fit the budget, down to one row per chunk.  The last chunk takes what is left.
struct RepackChunks { uint64_t chunk_rows, chunks; };
inline RepackChunks plan_repack_chunks(uint64_t budget_bytes, uint64_t nrows, uint64_t dst_words, uint64_t max_width)
{
	if(budget_bytes == 0){ budget_bytes = BUILD_DEFAULT_BUDGET_BYTES; }
	RepackChunks c;
	c.chunk_rows = nrows;
	while(c.chunk_rows > 1 && (c.chunk_rows*dst_words*4 > budget_bytes || c.chunk_rows*max_width > budget_bytes)){ c.chunk_rows /= 2; }
	c.chunks = c.chunk_rows ? (nrows + c.chunk_rows - 1)/c.chunk_rows : 0;
	return c;
}

}  // namespace kwage

#endif
