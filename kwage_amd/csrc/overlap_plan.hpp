// kwage_amd/csrc/overlap_plan.hpp -- the host-side planning of the overlap matrix (overlap.hip,
// kwage_group_column_overlaps): the refusals, the blocks of 32 columns either list is cut into (straight: one dword of the
// row; gathered: up to 32 columns from anywhere in the row), the workgroup tiles and their order, the parts the row range
// is cut into, and -- written ONCE for the kernel and the host -- what a lane stages of a block and how a word of staged
// bits spreads into the 0/1 bytes the matrix cores multiply.  Plain functions of plain values: no device, no group --
// tests/sanitize/overlap_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_OVERLAP_PLAN_HPP
#define KWAGE_AMD_OVERLAP_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "copy_plan.hpp"

namespace kwage {

constexpr uint32_t OVERLAP_BLOCK = 32;             // columns of a block: one operand block of the 32 x 32 x 32 product
constexpr uint32_t OVERLAP_TILE_BLOCKS = 4;        // blocks on either side of a workgroup tile
constexpr uint32_t OVERLAP_TILE = OVERLAP_BLOCK*OVERLAP_TILE_BLOCKS;      // 128 columns: one 16-byte unit of a row where straight
constexpr uint32_t OVERLAP_TILE_CELLS = OVERLAP_TILE*OVERLAP_TILE;
constexpr uint32_t OVERLAP_STEP_GROUPS = 32;       // groups of 32 rows a workgroup stages together: a step is 1024 rows
constexpr uint32_t OVERLAP_SUPER = 16;             // tiles on either side of a square of the schedule (below)
constexpr uint32_t OVERLAP_MAX_SPLITS = 256;       // most parts the plan cuts the row range into by itself
constexpr uint32_t OVERLAP_NO_COLUMN = 0xFFFFFFFFu;

// One block of a list.  straight: the 32 columns are columns 32 dword .. 32 dword + 31 of the row in this order, of which
// the bits of `mask` count (the valid mask's dword; in a NULL list also nothing at or beyond the span).  Gathered:
// column[p] is the column at place p of the block, OVERLAP_NO_COLUMN where the list ended (it yields zero).  144 bytes.
struct OverlapBlock {
	uint32_t straight, dword, mask, reserved;
	uint32_t column[OVERLAP_BLOCK];
};

// Workgroup tile (ta, tb): places 128 ta .. of a's list against places 128 tb .. of b's.
struct OverlapTile { uint32_t ta, tb; };

struct OverlapPlan {
	uint64_t n_a = 0, n_b = 0, rows = 0;
	uint64_t groups = 0;               // groups of 32 rows: ceil(rows / 32)
	uint32_t splits = 1;               // part p takes the groups [groups p / splits, groups (p + 1) / splits)
	uint32_t symmetric = 0;
	uint64_t straight_blocks = 0, gathered_blocks = 0;
	std::vector<OverlapBlock> blocks_a, blocks_b;      // (symmetric: blocks_b is empty, a's serve both sides)
	std::vector<OverlapTile> tiles;
};

// What a launch of the kernels (overlap_kernels.hpp) is told: plain values, filled by overlap.hip and neighbors.hip.
struct OverlapArgs {
	const uint8_t *a_bits, *b_bits;
	unsigned long long a_stride, b_stride;
	unsigned long long rows, groups;           // rows of both matrices; groups of 32 rows
	const OverlapBlock *blocks_a, *blocks_b;   // overlap_plan.hpp (symmetric: the same table)
	uint32_t n_blocks_a, n_blocks_b;
	const OverlapTile *tiles;
	uint32_t n_tiles, splits;
	unsigned long long n_a, n_b;               // cells: n_a x n_b
	uint32_t symmetric;
	uint32_t *cells;
	unsigned long long row_elems;
	uint32_t *partial;                         // splits > 1: [part][tile][128][128]
};

// What the refusals need to know of a call besides the two sides (copy_plan.hpp CopySide).
struct OverlapCall {
	bool have_cells, have_cols_a, have_cols_b;
	uint64_t n_a, n_b;                 // as given
	uint64_t span_a, span_b;           // the groups' spans (0 for a NULL group)
	uint64_t row_elems;
	bool search_pending;
};

// Cells in a row of the result: b's list, or b's span for a NULL list; in the symmetric form a's.
inline uint64_t overlap_row_cells(const OverlapCall &c, bool have_b)
{
	if(!have_b){ return c.have_cols_a ? c.n_a : c.span_a; }
	return c.have_cols_b ? c.n_b : c.span_b;
}

// The refusals of kwage_group_column_overlaps that need no look at a column, in the order the call makes them; a and b may
// be NULL (b == NULL is the symmetric form).  (The pending search is KWAGE_ERR_STATE, everything else KWAGE_ERR_ARG.)
inline int overlap_refusal(const char *who, const CopySide *a, const CopySide *b, const OverlapCall &c)
{
	if(!a || !c.have_cells){ return fail(KWAGE_ERR_ARG, "%s: NULL %s", who, !a ? "a" : "cells"); }
	if(!c.have_cols_a && c.n_a != 0){ return fail(KWAGE_ERR_ARG, "%s: NULL cols_a with n_a = %llu", who, (unsigned long long)c.n_a); }
	if(c.have_cols_a && c.n_a == 0){ return fail(KWAGE_ERR_ARG, "%s: n_a is 0", who); }
	if(!c.have_cols_b && c.n_b != 0){ return fail(KWAGE_ERR_ARG, "%s: NULL cols_b with n_b = %llu", who, (unsigned long long)c.n_b); }
	if(c.have_cols_b && c.n_b == 0){ return fail(KWAGE_ERR_ARG, "%s: n_b is 0", who); }
	if(!b && c.have_cols_b){ return fail(KWAGE_ERR_ARG, "%s: cols_b without b (the symmetric form takes a's list on both sides)", who); }
	if(b){
		if(a->ctx != b->ctx){ return fail(KWAGE_ERR_ARG, "%s: the groups belong to different contexts", who); }
		if(a->sparse || b->sparse){ return fail(KWAGE_ERR_ARG, "%s: a sparse group takes part in no overlap", who); }
		const kwage_params &p = a->params, &q = b->params;
		if(p.kmer_len != q.kmer_len){ return fail(KWAGE_ERR_ARG, "%s: kmer_len differs: a %u, b %u", who, p.kmer_len, q.kmer_len); }
		if(p.num_hash != q.num_hash){ return fail(KWAGE_ERR_ARG, "%s: num_hash differs: a %u, b %u", who, p.num_hash, q.num_hash); }
		if(p.log_2_filter_len != q.log_2_filter_len){ return fail(KWAGE_ERR_ARG, "%s: log_2_filter_len differs: a %u, b %u", who, p.log_2_filter_len, q.log_2_filter_len); }
		if(p.hash_func != q.hash_func){ return fail(KWAGE_ERR_ARG, "%s: hash_func differs: a %d, b %d", who, (int)p.hash_func, (int)q.hash_func); }
	}
	else if(a->sparse){ return fail(KWAGE_ERR_ARG, "%s: a sparse group takes part in no overlap", who); }
	if(a->params.log_2_filter_len >= 32){
		return fail(KWAGE_ERR_ARG, "%s: a filter of 2^32 rows is not supported (the set-bit count of a full one does not fit 32 bits)", who);
	}
	const uint64_t cells = overlap_row_cells(c, b != nullptr);
	if(c.row_elems < cells){ return fail(KWAGE_ERR_ARG, "%s: row_elems %llu is less than the %llu cells of a row", who, (unsigned long long)c.row_elems, (unsigned long long)cells); }
	if(c.search_pending){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); }
	return KWAGE_OK;
}

// A list's columns checked (save_plan.hpp save_check_columns' words, but a column may be listed twice): the first offender
// in list order.
inline int overlap_check_columns(const char *who, const uint64_t *columns, uint64_t n, uint64_t span, const uint8_t *valid)
{
	for(uint64_t i = 0; i < n; ++i){
		const uint64_t c = columns[i];
		if(c >= span){ return fail(KWAGE_ERR_ARG, "%s: column %llu is at or beyond the span %llu", who, (unsigned long long)c, (unsigned long long)span); }
		if(!((valid[c/8] >> (c%8)) & 1)){ return fail(KWAGE_ERR_ARG, "%s: column %llu is a pad or retired column", who, (unsigned long long)c); }
	}
	return KWAGE_OK;
}

// Dword `dword` of the valid mask (a bit per column, LSB first, (span + 7) / 8 bytes), zero beyond it.
inline uint32_t overlap_valid_dword(const uint8_t *valid, uint64_t span, uint64_t dword)
{
	const uint64_t bytes = (span + 7)/8;
	uint32_t v = 0;
	for(uint64_t j = 0; j < 4; ++j){ if(4*dword + j < bytes){ v |= (uint32_t)valid[4*dword + j] << (8*j); } }
	return v;
}

// One list (checked) cut into blocks.  columns == NULL: every column 0 .. span - 1, all blocks straight, dead columns
// masked out.  Otherwise a block is straight when it is full, starts at a multiple of 32 and goes on consecutively.
inline void overlap_cut_blocks(const uint64_t *columns, uint64_t n, uint64_t span, const uint8_t *valid, std::vector<OverlapBlock> &blocks,
                               uint64_t *straight, uint64_t *gathered)
{
	blocks.clear();
	const uint64_t count = columns ? n : span;
	for(uint64_t first = 0; first < count; first += OVERLAP_BLOCK){
		const uint64_t len = std::min<uint64_t>(OVERLAP_BLOCK, count - first);
		OverlapBlock blk{};
		bool is_straight = !columns || (len == OVERLAP_BLOCK && columns[first] % OVERLAP_BLOCK == 0);
		for(uint64_t i = 1; columns && is_straight && i < len; ++i){ is_straight = columns[first + i] == columns[first] + i; }
		if(is_straight){
			const uint64_t dword = (columns ? columns[first] : first)/OVERLAP_BLOCK;
			blk.straight = 1;
			blk.dword = (uint32_t)dword;
			blk.mask = overlap_valid_dword(valid, span, dword);
			++*straight;
		}
		else{
			for(uint64_t i = 0; i < OVERLAP_BLOCK; ++i){ blk.column[i] = i < len ? (uint32_t)columns[first + i] : OVERLAP_NO_COLUMN; }
			++*gathered;
		}
		blocks.push_back(blk);
	}
}

// The tiles of ta_n x tb_n, squares of OVERLAP_SUPER x OVERLAP_SUPER tiles one after the other and row-major inside a
// square: the workgroups that run together then read 16 neighbouring 16-byte slices of a row on either side -- whole
// cache lines between them.  symmetric: only ta <= tb.
inline void overlap_schedule(uint64_t ta_n, uint64_t tb_n, bool symmetric, std::vector<OverlapTile> &tiles)
{
	tiles.clear();
	for(uint64_t sa = 0; sa < ta_n; sa += OVERLAP_SUPER){
		for(uint64_t sb = symmetric ? sa : 0; sb < tb_n; sb += OVERLAP_SUPER){
			for(uint64_t ta = sa; ta < std::min<uint64_t>(sa + OVERLAP_SUPER, ta_n); ++ta){
				for(uint64_t tb = sb; tb < std::min<uint64_t>(sb + OVERLAP_SUPER, tb_n); ++tb){
					if(!symmetric || ta <= tb){ tiles.push_back(OverlapTile{(uint32_t)ta, (uint32_t)tb}); }
				}
			}
		}
	}
}

// Parts of the row range: `knob` (overlap_splits) where it is not 0, else as many as bring the launch to two workgroups
// per compute unit, a part no shorter than one step; never more parts than groups of 32 rows.
inline uint32_t overlap_choose_splits(uint64_t tiles, uint64_t groups, uint32_t ncu, int64_t knob)
{
	if(tiles == 0 || groups == 0){ return 1; }
	uint64_t s;
	if(knob > 0){ s = (uint64_t)knob; }
	else{
		const uint64_t want = 2ull*std::max<uint32_t>(ncu, 1);
		s = tiles >= want ? 1 : (want + tiles - 1)/tiles;
		s = std::min<uint64_t>(s, std::max<uint64_t>(groups/OVERLAP_STEP_GROUPS, 1));
		s = std::min<uint64_t>(s, OVERLAP_MAX_SPLITS);
	}
	return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(s, groups), 1);
}

// First group of part `part` (part == splits: the end).
KWAGE_HD inline uint64_t overlap_part_begin(uint64_t groups, uint32_t splits, uint32_t part)
{
	return groups*part/splits;      // (groups < 2^27, part < 2^31)
}

// Both lists (overlap_refusal passed) checked and planned.  Refused (KWAGE_ERR_ARG, the plan's tables empty), in this
// order: a column of a's list, then of b's, at or beyond its span or a pad or retired column; a launch that does not fit
// a grid.  have_b false: the symmetric form.
inline int plan_overlap(const char *who, const uint64_t *cols_a, uint64_t n_a, uint64_t span_a, const uint8_t *valid_a,
                        bool have_b, const uint64_t *cols_b, uint64_t n_b, uint64_t span_b, const uint8_t *valid_b,
                        uint64_t rows, uint32_t ncu, int64_t knob, OverlapPlan &plan)
{
	plan = OverlapPlan();
	int rc;
	if(cols_a && (rc = overlap_check_columns(who, cols_a, n_a, span_a, valid_a))){ return rc; }
	if(have_b && cols_b && (rc = overlap_check_columns(who, cols_b, n_b, span_b, valid_b))){ return rc; }
	if(span_a >= OVERLAP_NO_COLUMN || (have_b && span_b >= OVERLAP_NO_COLUMN)){ return fail(KWAGE_ERR_ARG, "%s: a span of 2^32 - 1 columns and more does not fit a launch", who); }
	plan.n_a = cols_a ? n_a : span_a;
	plan.n_b = !have_b ? plan.n_a : cols_b ? n_b : span_b;
	plan.rows = rows;
	plan.groups = (rows + 31)/32;
	plan.symmetric = have_b ? 0 : 1;
	const uint64_t ta_n = (plan.n_a + OVERLAP_TILE - 1)/OVERLAP_TILE, tb_n = (plan.n_b + OVERLAP_TILE - 1)/OVERLAP_TILE;
	const uint64_t tiles = have_b ? ta_n*tb_n : ta_n*(ta_n + 1)/2;
	plan.splits = overlap_choose_splits(tiles, plan.groups, ncu, knob);
	// one workgroup per (tile, part); the combine kernel: one lane per cell of every tile
	if(tiles*plan.splits > 0x7FFFFFFFull || tiles*(OVERLAP_TILE_CELLS/256) > 0x7FFFFFFFull){
		const uint32_t parts = plan.splits;
		plan = OverlapPlan();
		return fail(KWAGE_ERR_ARG, "%s: %llu tiles in %u parts do not fit a grid", who, (unsigned long long)tiles, parts);
	}
	overlap_cut_blocks(cols_a, n_a, span_a, valid_a, plan.blocks_a, &plan.straight_blocks, &plan.gathered_blocks);
	if(have_b){ overlap_cut_blocks(cols_b, n_b, span_b, valid_b, plan.blocks_b, &plan.straight_blocks, &plan.gathered_blocks); }
	overlap_schedule(ta_n, tb_n, !have_b, plan.tiles);
	return KWAGE_OK;
}

// Bytes of the parts' partial tiles (none for one part).
inline uint64_t overlap_partial_bytes(const OverlapPlan &plan)
{
	return plan.splits > 1 ? (uint64_t)plan.splits*plan.tiles.size()*OVERLAP_TILE_CELLS*sizeof(uint32_t) : 0;
}

// ---- what a lane stages, and how it becomes an operand: shared by the kernel and the host ----

// The dwords `dword` of the 32 rows first_row .. first_row + 31 of a matrix (rows `stride` bytes apart), ANDed with
// `mask`; zero for rows at or beyond end_row.  load(byte offset) returns the aligned dword there.  All offsets in 64
// bits: row 2^32 - 1 of 12544-byte rows lies beyond 2^45.
KWAGE_HD inline uint64_t overlap_stage_offset(uint64_t row, uint64_t stride, uint32_t dword) { return row*stride + 4ull*dword; }

template <typename LOAD>
KWAGE_HD inline void overlap_stage_rows(LOAD &&load, uint64_t stride, uint32_t dword, uint32_t mask, uint64_t first_row, uint64_t end_row, uint32_t (&v)[32])
{
#if defined(__clang__)
#pragma unroll
#endif
	for(int i = 0; i < 32; ++i){ v[i] = first_row + (uint64_t)i < end_row ? load(overlap_stage_offset(first_row + (uint64_t)i, stride, dword)) : 0u; }
#if defined(__clang__)
#pragma unroll
#endif
	for(int i = 0; i < 32; ++i){ v[i] &= mask; }
}

// Bit `bit` of 32 staged row dwords as one word: bit i is row i's.
KWAGE_HD inline uint32_t overlap_column_word(const uint32_t (&v)[32], uint32_t bit)
{
	uint32_t w = 0;
#if defined(__clang__)
#pragma unroll
#endif
	for(int i = 0; i < 32; ++i){ w |= ((v[i] >> bit) & 1u) << i; }
	return w;
}

// The spreading: a word of 32 rows' bits of ONE column becomes the 2 x 16 bytes, each 0 or 1, that the two lanes of the
// column (half h = 0, 1 of the wave) hand to the 32 x 32 x 32 product as four dwords e = 0 .. 3.  Byte q of dword e of
// half h is bit 8 q + 4 h + e of the word: a shift and an AND per dword, and over h, e and q every bit stands in exactly
// one byte.  Both operands of a product are spread by this function, so which row of the 32 a byte position means is the
// same on both sides, and the sum over rows does not care about their order.
KWAGE_HD inline uint32_t overlap_spread(uint32_t word, uint32_t h, uint32_t e) { return (word >> (4u*h + e)) & 0x01010101u; }

}  // namespace kwage

#endif
