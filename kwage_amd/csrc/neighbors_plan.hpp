// kwage_amd/csrc/neighbors_plan.hpp -- the host-side planning of the nearest-neighbour lists (neighbors.hip,
// kwage_group_column_neighbors): the refusals, the strips a's list is cut into and what the overlap kernels are told per
// strip (overlap_plan.hpp's blocks, schedule and parts, in the a x b form), and -- written ONCE for the kernel and the
// host -- the key, the eligibility of a candidate and the steps of the exact radix select over (key, index).  Plain
// functions of plain values: no device, no group -- tests/sanitize/neighbors_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_NEIGHBORS_PLAN_HPP
#define KWAGE_AMD_NEIGHBORS_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "overlap_plan.hpp"

namespace kwage {

constexpr int64_t NEIGHBORS_STRIP_BYTES = 256ll << 20;     // default of the knob neighbors_strip_bytes
constexpr uint32_t NEIGHBORS_STRIP_UNIT = OVERLAP_TILE;    // a strip is a multiple of this many entries (or all of them)
constexpr uint32_t NEIGHBORS_NO_INDEX = 0xFFFFFFFFu;       // index of a filler record
constexpr uint32_t NEIGHBORS_KEY_TOP_SHARED = 7;           // highest byte of the composite (key: bytes 4 .. 11, tie: 0 .. 3) that can be set
constexpr uint32_t NEIGHBORS_KEY_TOP_JACCARD = 11;

// ---- the key, the eligibility and the select's steps: shared by the kernel and the host ----

// floor(s 2^64 / u) for s <= u <= 2^32, all ones for s == u, 0 for an empty union: strictly monotone in the fraction s / u,
// because two distinct fractions with denominators <= 2^32 differ by at least 2^-64.  Two 64-bit divisions.
KWAGE_HD inline uint64_t neighbors_jaccard_key(uint32_t s, uint64_t u)
{
	if(u == 0){ return 0; }
	if((uint64_t)s == u){ return ~0ull; }
	const uint64_t n1 = (uint64_t)s << 32;
	const uint64_t q1 = n1/u, r1 = n1%u;          // q1 < 2^32 (s < u), r1 < u <= 2^32
	const uint64_t q2 = (r1 << 32)/u;             // < 2^32
	return (q1 << 32) | q2;
}

// The scalar key of a pair: larger is better.
KWAGE_HD inline uint64_t neighbors_key(uint32_t metric, uint32_t shared, uint32_t bits_a, uint32_t bits_b)
{
	if(metric == KWAGE_NEIGHBORS_SHARED){ return shared; }
	return neighbors_jaccard_key(shared, (uint64_t)bits_a + bits_b - shared);
}

// Whether a candidate naming column col_b (OVERLAP_NO_COLUMN: a dead one) may stand in the list of an entry naming col_a.
// skip_same: KWAGE_NEIGHBORS_SKIP_SELF was given and both lists name columns of one group.
KWAGE_HD inline bool neighbors_eligible(uint32_t col_a, uint32_t col_b, uint32_t shared, uint32_t min_shared, bool skip_same)
{
	return col_a != OVERLAP_NO_COLUMN && col_b != OVERLAP_NO_COLUMN && shared >= min_shared && !(skip_same && col_a == col_b);
}

// The tie word of candidate j among candidates whose indices fit tie_bytes bytes: larger for the smaller index, so that
// (key, tie) descending is key descending, then index ascending.
KWAGE_HD inline uint32_t neighbors_tie_bytes(uint64_t n_b) { return n_b <= (1ull << 8) ? 1u : n_b <= (1ull << 16) ? 2u : n_b <= (1ull << 24) ? 3u : 4u; }
KWAGE_HD inline uint32_t neighbors_tie(uint32_t tie_bytes, uint32_t j) { return (tie_bytes >= 4 ? 0xFFFFFFFFu : (1u << (8*tie_bytes)) - 1u) - j; }

// The composite of a candidate is the 12 bytes (key << 32 | tie); the select walks them from the top: key bytes
// top .. 4, then tie bytes tie_bytes - 1 .. 0 (the tie bytes above are zero in every candidate).
KWAGE_HD inline int neighbors_next_byte(int byte, uint32_t tie_bytes) { return byte == 4 ? (int)tie_bytes - 1 : byte - 1; }
KWAGE_HD inline uint32_t neighbors_digit(uint64_t key, uint32_t tie, int byte)
{
	return byte >= 4 ? (uint32_t)(key >> (8*(byte - 4))) & 255u : (tie >> (8*byte)) & 255u;
}
// Whether the composite's bytes ABOVE `byte` equal the prefix's.
KWAGE_HD inline bool neighbors_prefix_match(uint64_t key, uint32_t tie, uint64_t pkey, uint32_t ptie, int byte)
{
	if(byte >= 4){
		const int sh = 8*(byte - 4) + 8;
		return sh >= 64 || (key >> sh) == (pkey >> sh);
	}
	const int sh = 8*byte + 8;
	return key == pkey && (sh >= 32 || (tie >> sh) == (ptie >> sh));
}
// The prefix with `digit` set at `byte`.
KWAGE_HD inline void neighbors_prefix_set(uint64_t &pkey, uint32_t &ptie, int byte, uint32_t digit)
{
	if(byte >= 4){ pkey |= (uint64_t)digit << (8*(byte - 4)); }
	else{ ptie |= digit << (8*byte); }
}
// One step of the select on a histogram of the digits at one byte among the candidates that match the prefix: the digit
// in which the want-th best lies, `want` reduced by the candidates above it.  Returns the digit.
KWAGE_HD inline uint32_t neighbors_pick_digit(const uint32_t *hist, uint32_t &want)
{
	uint32_t above = 0;
	int b = 255;
	for(; b > 0 && above + hist[b] < want; --b){ above += hist[b]; }
	want -= above;
	return (uint32_t)b;
}
// Whether composite (key, tie) is at or above the cut (tkey, ttie).
KWAGE_HD inline bool neighbors_wins(uint64_t key, uint32_t tie, uint64_t tkey, uint32_t ttie) { return key > tkey || (key == tkey && tie >= ttie); }
// Whether record x = (key, index) stands BEHIND record y in the output.
KWAGE_HD inline bool neighbors_behind(uint64_t xkey, uint32_t xindex, uint64_t ykey, uint32_t yindex) { return xkey < ykey || (xkey == ykey && xindex > yindex); }

// ---- strips ----

// Cells of a row of a strip's block: the candidates rounded up to a multiple of 4, so that every row starts at a 16-byte
// boundary of the block.
KWAGE_HD inline uint64_t neighbors_pitch(uint64_t n_b) { return (n_b + 3) & ~3ull; }
// Where cell (entry e of a strip, candidate j) lies in the strip's block, in cells: 64 bits -- a strip of 1152 rows of
// 2^20 cells passes 2^30 cells, 4 GiB.
KWAGE_HD inline uint64_t neighbors_cell_offset(uint64_t e, uint64_t pitch, uint64_t j) { return e*pitch + j; }

// Entries of a full strip: the largest multiple of 128 whose cells fit `budget` bytes, at least 128, at most n_a.
inline uint64_t neighbors_strip_entries(uint64_t n_a, uint64_t n_b, int64_t budget)
{
	const uint64_t row_bytes = std::max<uint64_t>(neighbors_pitch(n_b), 4)*sizeof(uint32_t);
	uint64_t e = (uint64_t)std::max<int64_t>(budget, 0)/row_bytes/NEIGHBORS_STRIP_UNIT*NEIGHBORS_STRIP_UNIT;
	e = std::max<uint64_t>(e, NEIGHBORS_STRIP_UNIT);
	return std::min(e, n_a);
}

// What the overlap kernels are told for a strip of `entries` entries: its tiles (a x b form) and the parts of the rows.
struct NeighborsShape {
	uint64_t entries = 0;
	uint32_t splits = 1;
	std::vector<OverlapTile> tiles;
};

struct NeighborsPlan {
	uint64_t n_a = 0, n_b = 0, rows = 0, groups = 0;
	uint64_t pitch = 0;                   // cells of a row of the strip's block
	uint64_t strips = 0, strip_entries = 0;
	uint64_t tiles = 0;                   // all strips together
	uint64_t partial_bytes = 0;           // the larger of the two shapes'
	uint32_t tie_bytes = 1;
	NeighborsShape full, last;            // the strips but the last; the last where it is shorter (else entries == 0)
	std::vector<OverlapBlock> blocks_a, blocks_b;   // of the whole lists; (b == NULL: blocks_b is empty, a's serve both sides)
	std::vector<uint32_t> col_a, col_b;   // the column an entry / a candidate names, OVERLAP_NO_COLUMN for a dead one; (b == NULL: col_b empty)
};

// Strip s: its first entry and its shape.
inline uint64_t neighbors_strip_first(const NeighborsPlan &p, uint64_t s) { return s*p.strip_entries; }
inline const NeighborsShape &neighbors_strip_shape(const NeighborsPlan &p, uint64_t s) { return s + 1 == p.strips && p.last.entries ? p.last : p.full; }

// What every neighbours call refuses first (KWAGE_ERR_ARG), before the overlap's refusals.
inline int neighbors_refusal(const char *who, bool have_a, bool have_out, bool have_counts, uint32_t k, uint32_t metric)
{
	if(!have_a || !have_out || !have_counts){ return fail(KWAGE_ERR_ARG, "%s: NULL %s", who, !have_a ? "a" : !have_out ? "out" : "counts"); }
	if(k < 1 || k > KWAGE_TOPK_MAX){ return fail(KWAGE_ERR_ARG, "%s: k = %u, 1 .. %u required", who, k, KWAGE_TOPK_MAX); }
	if(metric != KWAGE_NEIGHBORS_SHARED && metric != KWAGE_NEIGHBORS_JACCARD){ return fail(KWAGE_ERR_ARG, "%s: unknown metric %u", who, metric); }
	return KWAGE_OK;
}

inline void neighbors_columns_of(const uint64_t *cols, uint64_t n, uint64_t span, const uint8_t *valid, std::vector<uint32_t> &out)
{
	const uint64_t count = cols ? n : span;
	out.resize(count);
	for(uint64_t i = 0; i < count; ++i){
		const uint64_t c = cols ? cols[i] : i;
		out[i] = (valid[c/8] >> (c%8)) & 1 ? (uint32_t)c : OVERLAP_NO_COLUMN;
	}
}

inline int neighbors_shape(const char *who, uint64_t entries, uint64_t n_b, uint64_t groups, uint32_t ncu, int64_t knob, NeighborsShape &shape)
{
	shape = NeighborsShape();
	shape.entries = entries;
	const uint64_t ta_n = (entries + OVERLAP_TILE - 1)/OVERLAP_TILE, tb_n = (n_b + OVERLAP_TILE - 1)/OVERLAP_TILE;
	const uint64_t tiles = ta_n*tb_n;
	shape.splits = overlap_choose_splits(tiles, groups, ncu, knob);
	if(tiles*shape.splits > 0x7FFFFFFFull || tiles*(OVERLAP_TILE_CELLS/256) > 0x7FFFFFFFull){
		return fail(KWAGE_ERR_ARG, "%s: %llu tiles in %u parts do not fit a grid", who, (unsigned long long)tiles, shape.splits);
	}
	overlap_schedule(ta_n, tb_n, false, shape.tiles);
	return KWAGE_OK;
}

// Both lists (neighbors_refusal and overlap_refusal passed) checked and planned.  Refused (KWAGE_ERR_ARG) as plan_overlap
// refuses, in its order: a column of a's list, then of b's, at or beyond its span or dead; spans or a launch that do not fit
// a grid.  have_b false: a's list is also the candidate list.
inline int plan_neighbors(const char *who, const uint64_t *cols_a, uint64_t n_a, uint64_t span_a, const uint8_t *valid_a,
                          bool have_b, const uint64_t *cols_b, uint64_t n_b, uint64_t span_b, const uint8_t *valid_b,
                          uint64_t rows, uint32_t ncu, int64_t splits_knob, int64_t strip_bytes, NeighborsPlan &plan)
{
	plan = NeighborsPlan();
	int rc;
	if(cols_a && (rc = overlap_check_columns(who, cols_a, n_a, span_a, valid_a))){ return rc; }
	if(have_b && cols_b && (rc = overlap_check_columns(who, cols_b, n_b, span_b, valid_b))){ return rc; }
	if(span_a >= OVERLAP_NO_COLUMN || (have_b && span_b >= OVERLAP_NO_COLUMN)){ return fail(KWAGE_ERR_ARG, "%s: a span of 2^32 - 1 columns and more does not fit a launch", who); }
	plan.n_a = cols_a ? n_a : span_a;
	plan.n_b = !have_b ? plan.n_a : cols_b ? n_b : span_b;
	plan.rows = rows;
	plan.groups = (rows + 31)/32;
	plan.pitch = neighbors_pitch(plan.n_b);
	plan.tie_bytes = neighbors_tie_bytes(plan.n_b);
	if(plan.n_a == 0){ return KWAGE_OK; }
	plan.strip_entries = neighbors_strip_entries(plan.n_a, plan.n_b, strip_bytes);
	plan.strips = (plan.n_a + plan.strip_entries - 1)/plan.strip_entries;
	const uint64_t rest = plan.n_a - (plan.strips - 1)*plan.strip_entries;
	if((rc = neighbors_shape(who, plan.strip_entries, plan.n_b, plan.groups, ncu, splits_knob, plan.full))
	   || (rest != plan.strip_entries && (rc = neighbors_shape(who, rest, plan.n_b, plan.groups, ncu, splits_knob, plan.last)))){
		plan = NeighborsPlan();
		return rc;
	}
	plan.tiles = (plan.strips - 1)*plan.full.tiles.size() + (plan.last.entries ? plan.last.tiles.size() : plan.full.tiles.size());
	for(const NeighborsShape *s : {&plan.full, &plan.last}){
		if(s->splits > 1){ plan.partial_bytes = std::max<uint64_t>(plan.partial_bytes, (uint64_t)s->splits*s->tiles.size()*OVERLAP_TILE_CELLS*sizeof(uint32_t)); }
	}
	uint64_t straight = 0, gathered = 0;
	overlap_cut_blocks(cols_a, n_a, span_a, valid_a, plan.blocks_a, &straight, &gathered);
	neighbors_columns_of(cols_a, n_a, span_a, valid_a, plan.col_a);
	if(have_b){
		overlap_cut_blocks(cols_b, n_b, span_b, valid_b, plan.blocks_b, &straight, &gathered);
		neighbors_columns_of(cols_b, n_b, span_b, valid_b, plan.col_b);
	}
	return KWAGE_OK;
}

// ---- one entry's list on the host, step by step as the kernel makes it (neighbors_kernels.hpp): the sanitizer test's ----

struct NeighborsRecord { uint32_t index, shared, bits_a, bits_b; };

// cell(j), column(j) and bits(column) are read only for j < n_b.  Returns the count; out[0, k) is written whole.
template <typename CELL, typename COLUMN, typename BITS>
inline uint32_t neighbors_select_entry(CELL &&cell, COLUMN &&column, BITS &&bits, uint64_t n_b, uint32_t col_a, uint32_t bits_a, uint32_t k, uint32_t metric,
                                       uint32_t min_shared, bool skip_same, NeighborsRecord *out)
{
	const uint32_t tie_bytes = neighbors_tie_bytes(n_b);
	auto visit = [&](auto &&f) {
		for(uint64_t j = 0; j < n_b; ++j){
			const uint32_t s = cell(j), cb = column(j);
			if(neighbors_eligible(col_a, cb, s, min_shared, skip_same)){ f((uint32_t)j, s, neighbors_key(metric, s, bits_a, bits(cb))); }
		}
	};
	uint64_t pkey = 0;
	uint32_t ptie = 0, want = k, eligible = 0;
	bool first = true, done = false;
	for(int byte = (int)(metric == KWAGE_NEIGHBORS_SHARED ? NEIGHBORS_KEY_TOP_SHARED : NEIGHBORS_KEY_TOP_JACCARD); byte >= 0 && !done; byte = neighbors_next_byte(byte, tie_bytes)){
		uint32_t hist[256] = {};
		visit([&](uint32_t j, uint32_t, uint64_t key) {
			const uint32_t tie = neighbors_tie(tie_bytes, j);
			if(neighbors_prefix_match(key, tie, pkey, ptie, byte)){ ++hist[neighbors_digit(key, tie, byte)]; }
		});
		if(first){
			for(uint32_t h : hist){ eligible += h; }
			first = false;
			if(eligible <= k){ break; }
		}
		const uint32_t d = neighbors_pick_digit(hist, want);
		neighbors_prefix_set(pkey, ptie, byte, d);
		done = hist[d] == want;
	}
	const uint32_t cnt = std::min(eligible, k);
	std::vector<uint64_t> wkey;
	std::vector<uint32_t> windex;
	visit([&](uint32_t j, uint32_t, uint64_t key) {
		if(neighbors_wins(key, neighbors_tie(tie_bytes, j), pkey, ptie)){ wkey.push_back(key); windex.push_back(j); }
	});
	if(wkey.size() != cnt){ return NEIGHBORS_NO_INDEX; }       // (the select is wrong: the caller's comparison says so)
	std::vector<uint32_t> order(cnt);
	for(uint32_t i = 0; i < cnt; ++i){ order[i] = i; }
	std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return neighbors_behind(wkey[y], windex[y], wkey[x], windex[x]); });
	for(uint32_t r = 0; r < k; ++r){
		if(r < cnt){
			const uint32_t j = windex[order[r]];
			out[r] = NeighborsRecord{j, cell(j), bits_a, bits(column(j))};
		}
		else{ out[r] = NeighborsRecord{NEIGHBORS_NO_INDEX, 0, 0, 0}; }
	}
	return cnt;
}

}  // namespace kwage

#endif
