// kwage_amd/csrc/save_plan.hpp -- the host-side planning of the save (save.hip, kwage_group_save_db): which columns may be
// saved, the runs a column list folds into, the rows of a staged chunk, and -- written ONCE for the kernel and the host --
// where a source column lies in the resident matrix and how a piece of a destination word is cut out of it.  Plain
// functions of plain values: no device, no group -- tests/sanitize/save_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_SAVE_PLAN_HPP
#define KWAGE_AMD_SAVE_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "internal.h"

#if defined(__HIPCC__)
#define KWAGE_HD __host__ __device__
#else
#define KWAGE_HD
#endif

namespace kwage {

// Destination columns dst_first .. dst_first + len - 1 of the file are source columns src_first .. src_first + len - 1 of
// the group.  The runs of a plan are sorted by dst_first and cover [0, n) without gaps.
struct SaveRun { uint64_t src_first; uint32_t dst_first; uint32_t len; };

// Where source column `src_column` of row `row` lies: the byte offset of the aligned dword that holds it (rows `stride`
// bytes apart, stride a multiple of 4) and the column's bit in that dword.  All in 64 bits: a matrix of 2^23 rows of
// 12544 bytes has offsets beyond 2^36.
struct SaveWindow { uint64_t byte; uint32_t shift; };
KWAGE_HD inline SaveWindow save_window(uint64_t row, uint64_t stride, uint64_t src_column)
{
	SaveWindow w;
	w.byte = row*stride + src_column/32*4;
	w.shift = (uint32_t)(src_column % 32);
	return w;
}

// `cnt` (1 .. 32) consecutive source columns from src_column on, of one row, as the low bits of a word; the bits above
// them are zero.  A funnel shift over two aligned dwords: the second one is loaded only where the piece reaches into it
// and where it lies inside the matrix (matrix_bytes = nrows * stride).  load(byte offset) returns the dword there.
template <typename LOAD>
KWAGE_HD inline uint32_t save_piece(LOAD &&load, uint64_t row, uint64_t stride, uint64_t matrix_bytes, uint64_t src_column, uint32_t cnt)
{
	const SaveWindow w = save_window(row, stride, src_column);
	const uint32_t lo = load(w.byte);
	uint32_t hi = 0;
	if(w.shift + cnt > 32 && w.byte + 8 <= matrix_bytes){ hi = load(w.byte + 4); }
	const uint64_t v = ((uint64_t)lo | ((uint64_t)hi << 32)) >> w.shift;
	return (uint32_t)v & (cnt >= 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u));
}

// The run that covers destination column d (d < n): the last one with dst_first <= d.
KWAGE_HD inline uint32_t save_find_run(const SaveRun *runs, uint32_t n_runs, uint32_t d)
{
	uint32_t lo = 0, hi = n_runs;
	while(hi - lo > 1){
		const uint32_t mid = lo + (hi - lo)/2;
		if(runs[mid].dst_first <= d){ lo = mid; } else { hi = mid; }
	}
	return lo;
}

// Destination bits [d0, d1) of one row (d1 - d0 <= 32, d1 <= n; d0 a multiple of 32 in the save and the compaction, any
// column in the copy between groups) as a word, bit d - d0 = destination column d; *k = the run that covers d0 on entry
// and the one that covers d1 (if any) on return.  The kernel's inner loop.
template <typename LOAD>
KWAGE_HD inline uint32_t save_word(LOAD &&load, const SaveRun *runs, uint32_t *k, uint64_t row, uint64_t stride, uint64_t matrix_bytes, uint32_t d0, uint32_t d1)
{
	uint32_t word = 0, d = d0;
	while(d < d1){
		const SaveRun r = runs[*k];
		const uint32_t off = d - r.dst_first;
		const uint32_t cnt = std::min(r.len - off, d1 - d);
		word |= save_piece(load, row, stride, matrix_bytes, r.src_first + off, cnt) << (d - d0);
		d += cnt;
		if(off + cnt == r.len){ ++*k; }
	}
	return word;
}

// A whole 16-byte unit that lies inside ONE run: destination columns d .. d + 127 are source columns src_column ..
// src_column + 127 of the row.  Nothing here depends on a loaded value, so the unit's loads are requested together: four
// consecutive source dwords -- as one 16-byte load, load4, where they start on a 16-byte boundary -- and a fifth only
// where the columns do not start on a dword boundary (the last column then lies in it: it is inside the matrix).
struct SaveQuad { uint32_t x, y, z, w; };
template <typename LOAD, typename LOAD4>
KWAGE_HD inline void save_unit_in_run(LOAD &&load, LOAD4 &&load4, uint64_t row, uint64_t stride, uint64_t src_column, uint32_t (&w)[4])
{
	const SaveWindow win = save_window(row, stride, src_column);
	uint32_t a[5];
	if(win.byte % 16 == 0){
		const SaveQuad q = load4(win.byte);
		a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
	}
	else{
		for(int j = 0; j < 4; ++j){ a[j] = load(win.byte + 4*j); }
	}
	a[4] = win.shift ? load(win.byte + 16) : 0u;
	for(int j = 0; j < 4; ++j){ w[j] = (uint32_t)(((uint64_t)a[j] | ((uint64_t)a[j + 1] << 32)) >> win.shift); }
}

// The column list of a save folded into runs, in list order: destination column i is source column columns[i].  Refused
// (KWAGE_ERR_ARG, `runs` empty): n == 0 or n > 2^32 - 1 (num_filter is a uint32_t), a column at or beyond the span, a
// pad or retired column of valid[] (the group's host valid mask, a bit per column, LSB first), a column named twice.
// The column checks and the folding are shared with the copy between groups (copy_plan.hpp plan_copy), which names itself
// in `who`.
inline int save_check_columns(const char *who, const uint64_t *columns, uint64_t n, uint64_t span, const uint8_t *valid)
{
	std::vector<uint8_t> seen((span + 7)/8, 0);
	for(uint64_t i = 0; i < n; ++i){
		const uint64_t c = columns[i];
		if(c >= span){ return fail(KWAGE_ERR_ARG, "%s: column %llu is at or beyond the span %llu", who, (unsigned long long)c, (unsigned long long)span); }
		if(!((valid[c/8] >> (c%8)) & 1)){ return fail(KWAGE_ERR_ARG, "%s: column %llu is a pad or retired column", who, (unsigned long long)c); }
		if((seen[c/8] >> (c%8)) & 1){ return fail(KWAGE_ERR_ARG, "%s: column %llu is listed twice", who, (unsigned long long)c); }
		seen[c/8] |= (uint8_t)(1u << (c%8));
	}
	return KWAGE_OK;
}
inline void save_fold_runs(const uint64_t *columns, uint64_t n, std::vector<SaveRun> &runs)
{
	runs.clear();
	for(uint64_t i = 0; i < n; ++i){
		if(!runs.empty() && columns[i] == runs.back().src_first + runs.back().len){ ++runs.back().len; }
		else{ runs.push_back(SaveRun{columns[i], (uint32_t)i, 1u}); }
	}
}
inline int plan_save(const uint64_t *columns, uint64_t n, uint64_t span, const uint8_t *valid, std::vector<SaveRun> &runs)
{
	const char *who = "kwage_group_save_db";
	runs.clear();
	if(n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(n > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: %llu columns do not fit num_filter", who, (unsigned long long)n); }
	const int rc = save_check_columns(who, columns, n, span, valid);
	if(rc){ return rc; }
	save_fold_runs(columns, n, runs);
	return KWAGE_OK;
}

// Rows per staged chunk and the chunks of a save: a chunk's output (rows x out_slice bytes, out_slice = ceil(n / 8)) fits
// `staging_bytes`, down to one row per chunk; 0 means 64 MiB.
struct SaveChunks { uint64_t out_slice, rows, chunks; };
inline SaveChunks plan_chunks(uint64_t staging_bytes, uint64_t n, uint64_t nrows)
{
	SaveChunks c;
	c.out_slice = (n + 7)/8;
	if(staging_bytes == 0){ staging_bytes = 64ull << 20; }
	c.rows = std::min<uint64_t>(std::max<uint64_t>(1, staging_bytes/c.out_slice), std::max<uint64_t>(nrows, 1));
	c.chunks = (nrows + c.rows - 1)/c.rows;
	return c;
}

}  // namespace kwage

#endif
