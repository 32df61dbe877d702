// tests/sanitize/overlap_sanitize.cpp -- the host-side planning of the overlap matrix (kwage_amd/csrc/overlap_plan.hpp: the
// refusals, the blocks, the tile and split schedules, the staging functions and the spreading the kernel shares with the
// host) under -fsanitize=address,undefined.  No device: the kernel's workgroups are walked on the host -- every lane's
// staging loads over matrices whose allocations end where the matrices end, the spread operands multiplied byte by byte
// as the 32 x 32 x 32 product multiplies them, partial tiles and their combination -- and the cells, sentinels around
// them, are compared with a bit-by-bit count.
//   overlap_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <vector>

#include "overlap_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, straight_seen = 0, gathered_seen = 0, mirrored = 0, split_cases = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

static const char *WHO = "kwage_group_column_overlaps";
static const uint32_t SENTINEL = 0xDEADBEEFu;

// A matrix of nrows rows of `stride` bytes in an allocation of EXACTLY nrows * stride bytes, every bit random: the dead
// columns below the span too (they must not count) and everything above the span.
struct Matrix {
	uint64_t nrows, stride, span;
	std::vector<uint8_t> bytes, valid;
	Matrix(uint64_t r, uint64_t s, uint64_t sp, const std::vector<uint64_t> &dead, std::mt19937_64 &rng) : nrows(r), stride(s), span(sp), bytes(r*s, 0), valid(s, 0)
	{
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
		for(uint64_t c : dead){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
		for(uint8_t &b : bytes){ b = (uint8_t)rng(); }
		// the restatement's view: every column below the span as a string of bits, taken bit by bit
		columns.assign(span, std::vector<uint64_t>((nrows + 63)/64, 0));
		for(uint64_t c = 0; c < span; ++c){
			for(uint64_t row = 0; row < nrows; ++row){ if(bit(row, c)){ columns[c][row/64] |= 1ull << (row%64); } }
		}
	}
	std::vector<std::vector<uint64_t>> columns;
	uint32_t shared(uint64_t ca, const Matrix &o, uint64_t cb) const
	{
		uint32_t n = 0;
		for(size_t w = 0; w < columns[ca].size(); ++w){ n += (uint32_t)__builtin_popcountll(columns[ca][w] & o.columns[cb][w]); }
		return n;
	}
	bool live(uint64_t c) const { return c < span && ((valid[c/8] >> (c%8)) & 1); }
	bool bit(uint64_t row, uint64_t c) const { return (bytes[row*stride + c/8] >> (c%8)) & 1; }
};

// The kernel's workgroup (tile, part) on the host: staging lane by lane, then the products.  acc[128][128].
static int walk_workgroup(const OverlapPlan &plan, const Matrix &ma, const Matrix &mb, uint32_t tile, uint32_t part, std::vector<uint32_t> &acc, bool *in_bounds)
{
	const std::vector<OverlapBlock> &ba = plan.blocks_a, &bb = plan.symmetric ? plan.blocks_a : plan.blocks_b;
	const OverlapTile tl = plan.tiles[tile];
	const uint64_t g_begin = overlap_part_begin(plan.groups, plan.splits, part), g_end = overlap_part_begin(plan.groups, plan.splits, part + 1);
	EXPECT(g_begin <= g_end && g_end <= plan.groups);
	acc.assign(OVERLAP_TILE_CELLS, 0);
	std::vector<uint32_t> lds(2*OVERLAP_TILE_BLOCKS*OVERLAP_STEP_GROUPS*OVERLAP_BLOCK);
	for(uint64_t g0 = g_begin; g0 < g_end; g0 += OVERLAP_STEP_GROUPS){
		std::fill(lds.begin(), lds.end(), 0xFFFFFFFFu);      // (whatever the last step left: every word is written again)
		for(uint32_t t = 0; t < 256; ++t){
			const uint32_t sblock = t >> 5, sgroup = t & 31;
			const bool side_b = sblock >= OVERLAP_TILE_BLOCKS;
			const std::vector<OverlapBlock> &blocks = side_b ? bb : ba;
			const Matrix &m = side_b ? mb : ma;
			const uint32_t bi = (side_b ? tl.tb : tl.ta)*OVERLAP_TILE_BLOCKS + (sblock & 3);
			uint32_t *stage = &lds[(sblock*OVERLAP_STEP_GROUPS + sgroup)*OVERLAP_BLOCK];
			const uint64_t group = g0 + sgroup, first_row = group*32, end_row = group < g_end ? plan.rows : 0;
			auto load = [&](uint64_t byte) {
				if(byte + 4 > m.bytes.size()){ *in_bounds = false; return 0u; }
				uint32_t v;
				memcpy(&v, m.bytes.data() + byte, 4);      // (little-endian hosts only, as the library)
				return v;
			};
			uint32_t v[32];
			if(bi >= blocks.size()){ for(int c = 0; c < 32; ++c){ stage[c] = 0; } }
			else if(blocks[bi].straight){
				overlap_stage_rows(load, m.stride, blocks[bi].dword, blocks[bi].mask, first_row, end_row, v);
				for(int c = 0; c < 32; ++c){ stage[c] = overlap_column_word(v, (uint32_t)c); }      // (the kernel: the transpose in registers)
			}
			else{
				uint32_t cur = OVERLAP_NO_COLUMN;
				for(uint32_t c = 0; c < OVERLAP_BLOCK; ++c){
					const uint32_t column = blocks[bi].column[c];
					uint32_t w = 0;
					if(column != OVERLAP_NO_COLUMN){
						if(column/32 != cur){ cur = column/32; overlap_stage_rows(load, m.stride, cur, 0xFFFFFFFFu, first_row, end_row, v); }
						w = overlap_column_word(v, column%32);
					}
					stage[c] = w;
				}
			}
		}
		const uint32_t steps = (uint32_t)std::min<uint64_t>(OVERLAP_STEP_GROUPS, g_end - g0);
		for(uint32_t g = 0; g < steps; ++g){
			for(uint32_t i = 0; i < OVERLAP_TILE; ++i){
				const uint32_t wa = lds[((i/32)*OVERLAP_STEP_GROUPS + g)*OVERLAP_BLOCK + i%32];
				for(uint32_t j = 0; j < OVERLAP_TILE; ++j){
					const uint32_t wb = lds[((4 + j/32)*OVERLAP_STEP_GROUPS + g)*OVERLAP_BLOCK + j%32];
					uint32_t sum = 0;      // the product's sum over k: the two halves' four dwords of 0 / 1 bytes, byte by byte
					for(uint32_t h = 0; h < 2; ++h){
						for(uint32_t e = 0; e < 4; ++e){ sum += (uint32_t)__builtin_popcount(overlap_spread(wa, h, e) & overlap_spread(wb, h, e)); }
					}
					acc[i*OVERLAP_TILE + j] += sum;
				}
			}
		}
	}
	return 0;
}

typedef std::vector<uint64_t> List;

// One call: a's list against b's (mb == nullptr: the symmetric form) in `knob` parts.
static int check_call(const Matrix &ma, const List *la, const Matrix *mb, const List *lb, int64_t knob, uint32_t ncu, uint64_t pad, std::mt19937_64 &rng)
{
	OverlapPlan plan;
	const Matrix &mbb = mb ? *mb : ma;
	EXPECT(plan_overlap(WHO, la ? la->data() : nullptr, la ? la->size() : 0, ma.span, ma.valid.data(), mb != nullptr,
	                    lb ? lb->data() : nullptr, lb ? lb->size() : 0, mbb.span, mbb.valid.data(), ma.nrows, ncu, knob, plan) == KWAGE_OK);
	const uint64_t n_a = la ? la->size() : ma.span, n_b = !mb ? n_a : lb ? lb->size() : mb->span;
	EXPECT(plan.n_a == n_a && plan.n_b == n_b && plan.rows == ma.nrows && plan.groups == (ma.nrows + 31)/32 && plan.symmetric == (mb ? 0u : 1u));
	EXPECT(plan.blocks_a.size() == (n_a + 31)/32 && plan.blocks_b.size() == (mb ? (n_b + 31)/32 : 0));
	EXPECT(plan.straight_blocks + plan.gathered_blocks == plan.blocks_a.size() + plan.blocks_b.size());
	EXPECT(plan.splits >= 1 && (plan.groups == 0 || plan.splits <= plan.groups));
	if(knob > 0 && plan.groups){ EXPECT(plan.splits == std::min<uint64_t>((uint64_t)knob, plan.groups)); }
	straight_seen += (long)plan.straight_blocks; gathered_seen += (long)plan.gathered_blocks;
	if(plan.splits > 1){ ++split_cases; }
	// the blocks say the list
	for(int side = 0; side < (mb ? 2 : 1); ++side){
		const std::vector<OverlapBlock> &blocks = side ? plan.blocks_b : plan.blocks_a;
		const List *l = side ? lb : la;
		const Matrix &m = side ? mbb : ma;
		const uint64_t n = side ? n_b : n_a;
		for(uint64_t p = 0; p < blocks.size()*32; ++p){
			const OverlapBlock &blk = blocks[p/32];
			const uint64_t want = p >= n ? ~0ull : l ? (*l)[p] : p;
			if(blk.straight){
				EXPECT(want == ~0ull || want == 32ull*blk.dword + p%32);
				EXPECT(((blk.mask >> (p%32)) & 1) == (want != ~0ull && m.live(want) ? 1u : 0u) || (want == ~0ull && l == nullptr));
				if(l){ EXPECT((*l)[p/32*32] % 32 == 0 && p/32*32 + 32 <= n); }
			}
			else{ EXPECT(l && blk.column[p%32] == (want == ~0ull ? OVERLAP_NO_COLUMN : (uint32_t)want)); }
		}
	}
	// every (tile, part) once; tiles below the diagonal in no schedule, mirrors only in the symmetric form
	const uint64_t ta_n = (n_a + 127)/128, tb_n = (n_b + 127)/128;
	std::map<std::pair<uint32_t, uint32_t>, int> seen;
	for(const OverlapTile &t : plan.tiles){
		EXPECT(t.ta < ta_n && t.tb < tb_n && (mb || t.ta <= t.tb));
		EXPECT((seen[std::make_pair(t.ta, t.tb)]++) == 0);
	}
	EXPECT(plan.tiles.size() == (mb ? ta_n*tb_n : ta_n*(ta_n + 1)/2));
	std::vector<uint64_t> group_cover(plan.groups, 0);
	for(uint32_t p = 0; p < plan.splits; ++p){
		for(uint64_t g = overlap_part_begin(plan.groups, plan.splits, p); g < overlap_part_begin(plan.groups, plan.splits, p + 1); ++g){ ++group_cover[g]; }
	}
	for(uint64_t c : group_cover){ EXPECT(c == 1); }
	EXPECT(overlap_partial_bytes(plan) == (plan.splits > 1 ? plan.splits*plan.tiles.size()*65536ull : 0));
	// the cells, as the kernels write them: a store per cell, counted
	const uint64_t row_elems = n_b + pad;
	std::vector<uint32_t> cells(n_a*row_elems, SENTINEL);
	std::vector<uint8_t> stores(n_a*row_elems, 0);
	std::vector<uint32_t> acc, sum;
	bool in_bounds = true;
	for(uint32_t t = 0; t < plan.tiles.size(); ++t){
		sum.assign(OVERLAP_TILE_CELLS, 0);
		for(uint32_t p = 0; p < plan.splits; ++p){
			if(walk_workgroup(plan, ma, mbb, t, p, acc, &in_bounds)){ return 1; }
			for(uint32_t i = 0; i < OVERLAP_TILE_CELLS; ++i){ sum[i] += acc[i]; }
		}
		const OverlapTile tl = plan.tiles[t];
		const bool mirror = plan.symmetric && tl.ta != tl.tb;
		for(uint32_t i = 0; i < OVERLAP_TILE_CELLS; ++i){
			const uint64_t ia = 128ull*tl.ta + i/128, jb = 128ull*tl.tb + i%128;
			if(ia < n_a && jb < n_b){
				cells[ia*row_elems + jb] = sum[i]; ++stores[ia*row_elems + jb];
				if(mirror){ cells[jb*row_elems + ia] = sum[i]; ++stores[jb*row_elems + ia]; ++mirrored; }
			}
		}
	}
	EXPECT(in_bounds);
	for(uint64_t i = 0; i < n_a; ++i){
		const uint64_t ca = la ? (*la)[i] : i;
		for(uint64_t j = 0; j < row_elems; ++j){
			if(j >= n_b){ EXPECT(cells[i*row_elems + j] == SENTINEL && stores[i*row_elems + j] == 0); continue; }
			const uint64_t cb = !mb ? (la ? (*la)[j] : j) : lb ? (*lb)[j] : j;
			uint32_t want = 0;
			if(ma.live(ca) && mbb.live(cb)){ want = ma.shared(ca, mbb, cb); }
			EXPECT(stores[i*row_elems + j] == 1);
			EXPECT(cells[i*row_elems + j] == want);
		}
	}
	(void)rng;
	return 0;
}

static int check_refusals()
{
	kwage_params p{31, 3, 10, 0}, q = p;
	int ctx1 = 0, ctx2 = 0;
	CopySide a{&ctx1, false, p}, b{&ctx1, false, q};
	auto call = [](bool cells, bool ca, uint64_t na, bool cb, uint64_t nb, uint64_t row_elems, bool pending) {
		return OverlapCall{cells, ca, cb, na, nb, 64, 40, row_elems, pending};
	};
	auto refusal = [&](const CopySide *x, const CopySide *y, const OverlapCall &c, int want, const char *word) {
		const int rc = overlap_refusal(WHO, x, y, c);
		++refused;
		return rc == want && strstr(kwage_last_error(), word) && strstr(kwage_last_error(), WHO);
	};
	// in the order of the header comment: each case has everything LATER wrong as well
	const OverlapCall all_wrong = call(false, false, 5, false, 5, 0, true);
	EXPECT(refusal(nullptr, &b, all_wrong, KWAGE_ERR_ARG, "NULL a"));
	EXPECT(refusal(&a, &b, all_wrong, KWAGE_ERR_ARG, "NULL cells"));
	EXPECT(refusal(&a, &b, call(true, false, 5, true, 0, 0, true), KWAGE_ERR_ARG, "NULL cols_a with n_a = 5"));
	EXPECT(refusal(&a, &b, call(true, true, 0, true, 0, 0, true), KWAGE_ERR_ARG, "n_a is 0"));
	EXPECT(refusal(&a, &b, call(true, true, 3, false, 7, 0, true), KWAGE_ERR_ARG, "NULL cols_b with n_b = 7"));
	EXPECT(refusal(&a, &b, call(true, true, 3, true, 0, 0, true), KWAGE_ERR_ARG, "n_b is 0"));
	EXPECT(refusal(&a, nullptr, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "cols_b without b"));
	CopySide other_ctx{&ctx2, true, p};
	other_ctx.params.kmer_len = 21;
	EXPECT(refusal(&a, &other_ctx, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "different contexts"));
	CopySide sparse{&ctx1, true, p};
	sparse.params.kmer_len = 21;
	EXPECT(refusal(&a, &sparse, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "sparse"));
	EXPECT(refusal(&sparse, &a, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "sparse"));
	EXPECT(refusal(&sparse, nullptr, call(true, true, 3, false, 0, 0, true), KWAGE_ERR_ARG, "sparse"));
	CopySide d = b;
	d.params.kmer_len = 21; d.params.num_hash = 2; d.params.log_2_filter_len = 32; d.params.hash_func = 1;
	EXPECT(refusal(&a, &d, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "kmer_len differs"));
	d.params.kmer_len = 31;
	EXPECT(refusal(&a, &d, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "num_hash differs"));
	d.params.num_hash = 3;
	EXPECT(refusal(&a, &d, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "log_2_filter_len differs"));
	d.params.log_2_filter_len = 10;
	EXPECT(refusal(&a, &d, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "hash_func differs"));
	CopySide a32 = a, b32 = b;
	a32.params.log_2_filter_len = b32.params.log_2_filter_len = 32;
	EXPECT(refusal(&a32, &b32, call(true, true, 3, true, 2, 0, true), KWAGE_ERR_ARG, "2^32 rows"));
	EXPECT(refusal(&a32, nullptr, call(true, true, 3, false, 0, 0, true), KWAGE_ERR_ARG, "2^32 rows"));
	EXPECT(refusal(&a, &b, call(true, true, 3, true, 2, 1, true), KWAGE_ERR_ARG, "row_elems 1 is less than the 2 cells"));
	EXPECT(refusal(&a, &b, call(true, true, 3, false, 0, 39, true), KWAGE_ERR_ARG, "row_elems 39 is less than the 40 cells"));      // b's span
	EXPECT(refusal(&a, nullptr, call(true, true, 3, false, 0, 2, true), KWAGE_ERR_ARG, "less than the 3 cells"));                 // symmetric: a's list
	EXPECT(refusal(&a, nullptr, call(true, false, 0, false, 0, 63, true), KWAGE_ERR_ARG, "less than the 64 cells"));              // symmetric: a's span
	EXPECT(refusal(&a, &b, call(true, true, 3, true, 2, 2, true), KWAGE_ERR_STATE, "a search is pending"));
	EXPECT(overlap_refusal(WHO, &a, &b, call(true, true, 3, true, 2, 2, false)) == KWAGE_OK);
	EXPECT(overlap_refusal(WHO, &a, &a, call(true, false, 0, false, 0, 64, false)) == KWAGE_OK);
	EXPECT(overlap_refusal(WHO, &a, nullptr, call(true, false, 0, false, 0, 64, false)) == KWAGE_OK);
	// the columns: a's list before b's, the first offender in list order, a repeat allowed
	std::vector<uint8_t> valid(16, 0xFF);
	valid[1] &= (uint8_t)~2u;      // column 9 is dead
	OverlapPlan plan;
	auto plan_rc = [&](const List &la, const List &lb, const char *word) {
		const int rc = plan_overlap(WHO, la.data(), la.size(), 64, valid.data(), true, lb.data(), lb.size(), 40, valid.data(), 1024, 8, 0, plan);
		++refused;
		return rc == KWAGE_ERR_ARG && strstr(kwage_last_error(), word) && plan.tiles.empty() && plan.blocks_a.empty();
	};
	EXPECT(plan_rc({1, 64, 9}, {40}, "column 64 is at or beyond the span 64"));
	EXPECT(plan_rc({1, 9, 64}, {40}, "column 9 is a pad or retired column"));
	EXPECT(plan_rc({1, 1}, {3, 40, 9}, "column 40 is at or beyond the span 40"));
	EXPECT(plan_rc({1, 1}, {3, 9, 40}, "column 9 is a pad or retired column"));
	EXPECT(plan_overlap(WHO, List{1, 1}.data(), 2, 64, valid.data(), true, List{3, 3}.data(), 2, 40, valid.data(), 1024, 8, 0, plan) == KWAGE_OK);
	// a launch that does not fit a grid: 2^18 x 2^18 columns are 2^22 tiles, in 1024 parts 2^32 workgroups
	std::vector<uint8_t> wide((1u << 18)/8, 0xFF);
	EXPECT(plan_overlap(WHO, nullptr, 0, 1u << 18, wide.data(), true, nullptr, 0, 1u << 18, wide.data(), 1u << 20, 8, 1024, plan) == KWAGE_ERR_ARG);
	++refused;
	EXPECT(strstr(kwage_last_error(), "do not fit a grid") && plan.tiles.empty());
	return 0;
}

static int check_spread()
{
	std::mt19937_64 rng(7);
	for(int t = 0; t < 2000; ++t){
		const uint32_t w = t == 0 ? 0u : t == 1 ? 0xFFFFFFFFu : t < 34 ? 1u << (t - 2) : (uint32_t)rng();
		uint32_t covered = 0;
		for(uint32_t h = 0; h < 2; ++h){
			for(uint32_t e = 0; e < 4; ++e){
				const uint32_t s = overlap_spread(w, h, e);
				for(uint32_t q = 0; q < 4; ++q){
					const uint32_t bit = 8*q + 4*h + e, byte = (s >> (8*q)) & 0xFFu;
					EXPECT(byte == ((w >> bit) & 1u));
					EXPECT(!((covered >> bit) & 1u));
					covered |= 1u << bit;
				}
			}
		}
		EXPECT(covered == 0xFFFFFFFFu);
	}
	return 0;
}

static int check_offsets()
{
	// row 2^32 - 1 of 12544-byte rows: beyond 2^45, pure arithmetic
	const uint64_t row = 0xFFFFFFFFull, stride = 12544;
	EXPECT(overlap_stage_offset(row, stride, 0) == 53876069748480ull);
	EXPECT(overlap_stage_offset(row, stride, 3135) == 53876069748480ull + 12540);
	EXPECT(overlap_stage_offset(row, stride, 3135) + 4 == (row + 1)*stride);
	EXPECT(overlap_part_begin(1ull << 26, 1u << 20, 1u << 20) == 1ull << 26);
	EXPECT(overlap_part_begin((1ull << 26) + 5, 3, 3) == (1ull << 26) + 5 && overlap_part_begin((1ull << 26) + 5, 3, 0) == 0);
	// the plan's own choice of parts
	EXPECT(overlap_choose_splits(2080, 1u << 18, 256, 0) == 1);
	EXPECT(overlap_choose_splits(1, 1u << 18, 256, 0) == OVERLAP_MAX_SPLITS);
	EXPECT(overlap_choose_splits(64, 1u << 18, 256, 0) == 8);
	EXPECT(overlap_choose_splits(1, 32, 256, 0) == 1 && overlap_choose_splits(1, 1, 256, 8) == 1 && overlap_choose_splits(1, 32, 256, 8) == 8);
	EXPECT(overlap_choose_splits(0, 32, 256, 8) == 1 && overlap_choose_splits(5, 0, 256, 0) == 1);
	return 0;
}

int main()
{
	std::mt19937_64 rng(20261021);
	if(check_refusals() || check_spread() || check_offsets()){ return 1; }
	// a: 300 columns in 48-byte rows (128-byte stride would hide an overrun: the allocation ends with the last row's
	// last byte), columns 9, 40 and 200 dead; b: 140 columns in 20-byte rows, column 33 dead
	for(uint32_t L : {0u, 3u, 5u, 6u, 10u}){
		const uint64_t rows = 1ull << L;
		Matrix ma(rows, 40, 300, {9, 40, 200}, rng), mb(rows, 20, 140, {33}, rng);
		List aligned(64), shifted(64), reversed(33), shuffle(129), repeat{5, 5, 7, 5}, mixed, one{299}, b_last{139}, all_b;
		std::iota(aligned.begin(), aligned.end(), 64);
		std::iota(shifted.begin(), shifted.end(), 65);
		for(uint64_t i = 0; i < reversed.size(); ++i){ reversed[i] = 139 - i; }
		for(uint64_t i = 0; i < shuffle.size(); ++i){ shuffle[i] = 41 + i; }
		std::shuffle(shuffle.begin(), shuffle.end(), rng);
		for(uint64_t i = 0; i < 32; ++i){ mixed.push_back(96 + i); }
		for(uint64_t i = 0; i < 32; ++i){ mixed.push_back(97 + 2*i); }
		for(uint64_t i = 0; i < 32; ++i){ mixed.push_back(256 + i); }
		mixed.push_back(0);
		for(uint64_t c = 0; c < 140; ++c){ if(c != 33){ all_b.push_back(c); } }
		const int64_t knobs[] = {0, 1, 2, 3, 8};
		for(int64_t knob : knobs){
			if(L != 10 && knob > 1){ continue; }
			if(check_call(ma, nullptr, nullptr, nullptr, knob, 8, 3, rng)){ return 1; }          // symmetric, every column
			if(check_call(ma, &shuffle, nullptr, nullptr, knob, 8, 0, rng)){ return 1; }         // symmetric, gathered, two tiles
			if(check_call(ma, nullptr, &mb, nullptr, knob, 8, 1, rng)){ return 1; }              // every column against every column
			if(check_call(ma, &mixed, &mb, &reversed, knob, 8, 2, rng)){ return 1; }
			if(check_call(mb, &all_b, &ma, &aligned, knob, 8, 0, rng)){ return 1; }
		}
		if(check_call(ma, &shifted, &ma, &aligned, 0, 8, 5, rng)){ return 1; }                   // b is a
		if(check_call(ma, &repeat, &mb, &b_last, 0, 256, 0, rng)){ return 1; }
		if(check_call(ma, &one, nullptr, nullptr, 0, 8, 0, rng)){ return 1; }
		if(check_call(ma, &aligned, nullptr, nullptr, 0, 1, 7, rng)){ return 1; }
	}
	// an empty group: nothing planned, nothing walked
	{
		Matrix empty(1024, 16, 0, {}, rng);
		if(check_call(empty, nullptr, nullptr, nullptr, 0, 8, 0, rng)){ return 1; }
		if(check_call(empty, nullptr, &empty, nullptr, 0, 8, 4, rng)){ return 1; }
	}
	if(!(straight_seen > 100 && gathered_seen > 100 && mirrored > 1000 && split_cases >= 15)){
		fprintf(stderr, "FAILED: too little covered: %ld straight, %ld gathered, %ld mirrored, %ld split\n", straight_seen, gathered_seen, mirrored, split_cases);
		return 1;
	}
	printf("sanitizers: %ld checks, %ld refusals, %ld straight and %ld gathered blocks, %ld mirrored cells, %ld calls in several parts: no report\n",
	       checks, refused, straight_seen, gathered_seen, mirrored, split_cases);
	return 0;
}
