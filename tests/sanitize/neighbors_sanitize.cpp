// tests/sanitize/neighbors_sanitize.cpp -- the host-side planning of the nearest-neighbour lists
// (kwage_amd/csrc/neighbors_plan.hpp over overlap_plan.hpp: the refusals, the strips, per strip the overlap's tiles and
// parts, the key, the eligibility and the steps of the radix select the kernel shares with the host) under
// -fsanitize=address,undefined.  No device: the strips are walked, the cells of a strip live in an allocation that ends
// where the strip's rows end, the select kernel's workgroup is walked lane by lane over them -- 16-byte loads, histograms,
// the cut, the winners, the bitonic order -- and every list is compared with a plain sort under the exact order.
//   neighbors_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "neighbors_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, lists = 0, strips_walked = 0, early_cuts = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

static const char *WHO = "kwage_group_column_neighbors";
static const uint32_t THREADS = 256;

static bool refusal(int rc, const char *word)
{
	++refused;
	return rc == KWAGE_ERR_ARG && strstr(kwage_last_error(), word) && strstr(kwage_last_error(), WHO);
}

struct Side {
	uint64_t span;
	std::vector<uint8_t> valid;
	std::vector<uint32_t> bits;         // per column
	Side(uint64_t sp, const std::vector<uint64_t> &dead, std::mt19937_64 &rng, uint32_t max_bits) : span(sp), valid((sp + 7)/8 + 1, 0), bits(sp)
	{
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); bits[c] = (uint32_t)(rng()%(max_bits + 1ull)); }
		for(uint64_t c : dead){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
	}
};

// Exact comparison of two candidates of one entry: x stands before y.
static bool before(uint32_t metric, uint32_t bits_a, uint32_t sx, uint32_t bx, uint32_t jx, uint32_t sy, uint32_t by, uint32_t jy)
{
	if(metric == KWAGE_NEIGHBORS_SHARED){
		if(sx != sy){ return sx > sy; }
	}
	else{
		const uint64_t ux = (uint64_t)bits_a + bx - sx, uy = (uint64_t)bits_a + by - sy;
		const unsigned __int128 l = (unsigned __int128)(ux ? sx : 0)*(uy ? uy : 1), r = (unsigned __int128)(uy ? sy : 0)*(ux ? ux : 1);
		if(l != r){ return l > r; }
	}
	return jx < jy;
}

// The select kernel's workgroup for one entry, lane by lane: `row` points at the entry's cells inside the strip's
// allocation; every lane's 16-byte load is a memcpy the sanitizer sees.
static int walk_entry(const uint32_t *row, uint64_t n_b, const std::vector<uint32_t> &col_b, const std::vector<uint32_t> &bits_b, uint32_t col_a, uint32_t bits_a,
                      uint32_t k, uint32_t metric, uint32_t min_shared, bool skip_same, std::vector<NeighborsRecord> &out, uint32_t *count)
{
	const uint32_t tie_bytes = neighbors_tie_bytes(n_b);
	auto visit = [&](auto &&f) {
		if(col_a == OVERLAP_NO_COLUMN){ return; }
		for(uint32_t tid = 0; tid < THREADS; ++tid){
			for(uint64_t j0 = 4ull*tid; j0 < n_b; j0 += 4ull*THREADS){
				uint32_t s[4];
				memcpy(s, row + j0, 16);
				for(int t = 0; t < 4; ++t){
					const uint64_t j = j0 + t;
					if(j < n_b && neighbors_eligible(col_a, col_b[j], s[t], min_shared, skip_same)){ f((uint32_t)j, neighbors_key(metric, s[t], bits_a, bits_b[col_b[j]])); }
				}
			}
		}
	};
	uint64_t pkey = 0;
	uint32_t ptie = 0, want = k, eligible = 0;
	bool first = true;
	int passes = 0;
	for(int byte = (int)(metric == KWAGE_NEIGHBORS_SHARED ? NEIGHBORS_KEY_TOP_SHARED : NEIGHBORS_KEY_TOP_JACCARD); byte >= 0; byte = neighbors_next_byte(byte, tie_bytes)){
		uint32_t hist[256] = {};
		++passes;
		visit([&](uint32_t j, uint64_t key) {
			const uint32_t tie = neighbors_tie(tie_bytes, j);
			if(neighbors_prefix_match(key, tie, pkey, ptie, byte)){ ++hist[neighbors_digit(key, tie, byte)]; }
		});
		bool done = false;
		if(first){
			for(uint32_t h : hist){ eligible += h; }
			done = eligible <= k;
			first = false;
		}
		if(!done){
			const uint32_t d = neighbors_pick_digit(hist, want);
			EXPECT(want >= 1 && hist[d] >= want);
			neighbors_prefix_set(pkey, ptie, byte, d);
			done = hist[d] == want;
		}
		if(done){ break; }
	}
	if(passes < (int)(metric == KWAGE_NEIGHBORS_SHARED ? 4 : 8) + (int)tie_bytes){ ++early_cuts; }
	const uint32_t cnt = std::min(eligible, k);
	uint32_t P = 1;
	while(P < cnt){ P <<= 1; }
	std::vector<uint64_t> wkey(P, 0);
	std::vector<uint32_t> windex(P, NEIGHBORS_NO_INDEX);
	uint32_t n = 0;
	visit([&](uint32_t j, uint64_t key) {
		if(neighbors_wins(key, neighbors_tie(tie_bytes, j), pkey, ptie)){
			if(n < cnt){ wkey[n] = key; windex[n] = j; }
			++n;
		}
	});
	EXPECT(n == cnt);
	for(uint32_t size = 2; size <= P; size <<= 1){
		for(uint32_t stride = size >> 1; stride > 0; stride >>= 1){
			for(uint32_t t = 0; t < P/2; ++t){
				const uint32_t lo = 2*t - (t & (stride - 1)), hi = lo + stride;
				const bool asc = (lo & size) == 0;
				EXPECT(hi < P);
				if(neighbors_behind(wkey[lo], windex[lo], wkey[hi], windex[hi]) == asc){ std::swap(wkey[lo], wkey[hi]); std::swap(windex[lo], windex[hi]); }
			}
		}
	}
	out.assign(k, NeighborsRecord{NEIGHBORS_NO_INDEX, 0, 0, 0});
	for(uint32_t r = 0; r < cnt; ++r){
		const uint32_t j = windex[r];
		EXPECT(j < n_b);
		out[r] = NeighborsRecord{j, row[j], bits_a, bits_b[col_b[j]]};
	}
	*count = cnt;
	return 0;
}

static bool same(const NeighborsRecord &x, const NeighborsRecord &y) { return x.index == y.index && x.shared == y.shared && x.bits_a == y.bits_a && x.bits_b == y.bits_b; }

// One call: the plan, its strips, every entry's list by the lane walk and by neighbors_select_entry against a plain sort.
static int one_call(std::mt19937_64 &rng, const Side &a, const uint64_t *cols_a, uint64_t n_a, const Side *b, const uint64_t *cols_b, uint64_t n_b,
                    uint32_t k, uint32_t metric, uint32_t min_shared, bool skip_self, int64_t strip_bytes, int64_t splits, uint32_t max_bits, int tie_mode)
{
	NeighborsPlan plan;
	const Side &sb = b ? *b : a;
	EXPECT(plan_neighbors(WHO, cols_a, n_a, a.span, a.valid.data(), b != nullptr, cols_b, n_b, sb.span, sb.valid.data(), 1ull << 10, 256, splits, strip_bytes, plan) == KWAGE_OK);
	const bool skip_same = skip_self && (!b || b == &a);
	const std::vector<uint32_t> &col_b = b ? plan.col_b : plan.col_a;
	EXPECT(plan.col_a.size() == plan.n_a && col_b.size() == plan.n_b && plan.pitch % 4 == 0 && plan.pitch >= plan.n_b && plan.pitch < plan.n_b + 4);
	if(plan.n_a == 0){ EXPECT(plan.strips == 0 && plan.tiles == 0); return 0; }
	EXPECT(plan.strip_entries <= plan.n_a && (plan.strip_entries % 128 == 0 || plan.strip_entries == plan.n_a) && plan.strip_entries >= std::min<uint64_t>(128, plan.n_a));
	EXPECT(plan.strip_entries == plan.n_a || (plan.strip_entries*plan.pitch*4 <= (uint64_t)std::max<int64_t>(strip_bytes, 0) || plan.strip_entries == 128));
	uint64_t covered = 0, tiles = 0;
	for(uint64_t s = 0; s < plan.strips; ++s){
		++strips_walked;
		const NeighborsShape &shape = neighbors_strip_shape(plan, s);
		const uint64_t first = neighbors_strip_first(plan, s);
		EXPECT(first == covered && shape.entries >= 1 && shape.entries <= plan.strip_entries && first % OVERLAP_TILE == 0);
		EXPECT(s + 1 == plan.strips || shape.entries == plan.strip_entries);
		covered += shape.entries;
		tiles += shape.tiles.size();
		// the strip's blocks of a's list lie inside the table, and every store of the overlap kernels inside the strip's block
		const uint64_t first_block = first/OVERLAP_BLOCK, n_blocks = (shape.entries + OVERLAP_BLOCK - 1)/OVERLAP_BLOCK;
		EXPECT(first_block + n_blocks <= plan.blocks_a.size());
		EXPECT(shape.splits >= 1 && (shape.splits == 1 || (uint64_t)shape.splits*shape.tiles.size()*OVERLAP_TILE_CELLS*4 <= plan.partial_bytes));
		// the cells of the strip: an allocation of exactly entries x pitch cells
		std::vector<uint32_t> cells(shape.entries*plan.pitch, 0xDEADBEEFu);
		std::vector<uint8_t> stored(shape.entries*plan.pitch, 0);
		for(const OverlapTile &tl : shape.tiles){
			for(uint32_t r = 0; r < OVERLAP_TILE; ++r){
				for(uint32_t c = 0; c < OVERLAP_TILE; ++c){
					const uint64_t ia = (uint64_t)tl.ta*OVERLAP_TILE + r, jb = (uint64_t)tl.tb*OVERLAP_TILE + c;
					if(ia < shape.entries && jb < plan.n_b){
						const uint64_t at = neighbors_cell_offset(ia, plan.pitch, jb);
						EXPECT(at < cells.size() && !stored[at]);
						stored[at] = 1;
						const uint32_t ca = plan.col_a[first + ia], cb = col_b[jb];
						uint32_t v = 0;
						if(ca != OVERLAP_NO_COLUMN && cb != OVERLAP_NO_COLUMN){
							const uint32_t top = std::min(a.bits[ca], sb.bits[cb]);
							v = tie_mode == 2 ? top : tie_mode == 1 ? (uint32_t)(rng()%3)*(top/2) : (uint32_t)(rng()%(top + 1ull));
							if(skip_same && ca == cb){ v = a.bits[ca]; }
						}
						cells[at] = v;
					}
				}
			}
		}
		for(uint64_t e = 0; e < shape.entries; ++e){
			for(uint64_t j = 0; j < plan.n_b; ++j){ EXPECT(stored[neighbors_cell_offset(e, plan.pitch, j)]); }
			const uint32_t ca = plan.col_a[first + e], ba = ca != OVERLAP_NO_COLUMN ? a.bits[ca] : 0;
			const uint32_t *row = cells.data() + neighbors_cell_offset(e, plan.pitch, 0);
			std::vector<NeighborsRecord> got, got2(k);
			uint32_t count = 0;
			if(walk_entry(row, plan.n_b, col_b, sb.bits, ca, ba, k, metric, min_shared, skip_same, got, &count)){ return 1; }
			const uint32_t count2 = neighbors_select_entry([&](uint64_t j) { return row[j]; }, [&](uint64_t j) { return col_b[j]; }, [&](uint32_t c) { return sb.bits[c]; },
			                                               plan.n_b, ca, ba, k, metric, min_shared, skip_same, got2.data());
			// the plain sort
			std::vector<uint32_t> want;
			for(uint64_t j = 0; j < plan.n_b; ++j){
				if(ca != OVERLAP_NO_COLUMN && col_b[j] != OVERLAP_NO_COLUMN && row[j] >= min_shared && !(skip_same && ca == col_b[j])){ want.push_back((uint32_t)j); }
			}
			std::sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return before(metric, ba, row[x], sb.bits[col_b[x]], x, row[y], sb.bits[col_b[y]], y); });
			EXPECT(count == std::min<uint64_t>(want.size(), k) && count2 == count);
			for(uint32_t r = 0; r < k; ++r){
				const NeighborsRecord w = r < count ? NeighborsRecord{want[r], row[want[r]], ba, sb.bits[col_b[want[r]]]} : NeighborsRecord{NEIGHBORS_NO_INDEX, 0, 0, 0};
				EXPECT(same(got[r], w) && same(got2[r], w));
			}
			++lists;
		}
	}
	EXPECT(covered == plan.n_a && tiles == plan.tiles);
	return 0;
}

static int run()
{
	std::mt19937_64 rng(20261021);
	// ---- the refusals of the call's own, in order
	EXPECT(refusal(neighbors_refusal(WHO, false, false, false, 0, 9), "NULL a"));
	EXPECT(refusal(neighbors_refusal(WHO, true, false, false, 0, 9), "NULL out"));
	EXPECT(refusal(neighbors_refusal(WHO, true, true, false, 0, 9), "NULL counts"));
	EXPECT(refusal(neighbors_refusal(WHO, true, true, true, 0, 9), "k = 0"));
	EXPECT(refusal(neighbors_refusal(WHO, true, true, true, KWAGE_TOPK_MAX + 1, 9), "k = 1025"));
	EXPECT(refusal(neighbors_refusal(WHO, true, true, true, KWAGE_TOPK_MAX, 2), "unknown metric 2"));
	EXPECT(neighbors_refusal(WHO, true, true, true, 1, KWAGE_NEIGHBORS_SHARED) == KWAGE_OK && neighbors_refusal(WHO, true, true, true, KWAGE_TOPK_MAX, KWAGE_NEIGHBORS_JACCARD) == KWAGE_OK);
	// ---- the planner's: a listed dead column, a column beyond the span (the overlap's words with this call's name)
	{
		Side a(300, {7, 130}, rng, 1000), b(50, {33}, rng, 1000);
		NeighborsPlan plan;
		const uint64_t dead[3] = {0, 130, 400}, beyond[2] = {1, 300}, good[2] = {1, 2}, dead_b[2] = {2, 33};
		EXPECT(refusal(plan_neighbors(WHO, dead, 3, a.span, a.valid.data(), false, nullptr, 0, 0, nullptr, 1024, 256, 0, 1 << 20, plan), "column 130 is a pad or retired column"));
		EXPECT(refusal(plan_neighbors(WHO, beyond, 2, a.span, a.valid.data(), true, dead_b, 2, b.span, b.valid.data(), 1024, 256, 0, 1 << 20, plan), "column 300 is at or beyond the span 300"));
		EXPECT(refusal(plan_neighbors(WHO, good, 2, a.span, a.valid.data(), true, dead_b, 2, b.span, b.valid.data(), 1024, 256, 0, 1 << 20, plan), "column 33 is a pad or retired column"));
		EXPECT(plan.n_a == 0 && plan.blocks_a.empty() && plan.full.tiles.empty());
		EXPECT(refusal(plan_neighbors(WHO, nullptr, 0, 0xFFFFFFFFull, a.valid.data(), false, nullptr, 0, 0, nullptr, 1024, 256, 0, 1 << 20, plan), "does not fit a launch"));
	}
	// ---- the key: monotone in the fraction on neighbours of the closest kind
	for(int t = 0; t < 20000; ++t){
		const uint64_t u = (1ull << 32) - rng()%1000, s = rng()%(std::min<uint64_t>(u, 1ull << 31) + 1);
		const uint64_t k0 = neighbors_jaccard_key((uint32_t)s, u);
		if(s + 1 <= u && s + 1 < (1ull << 32)){ EXPECT(neighbors_jaccard_key((uint32_t)(s + 1), u) > k0); }
		if(s < u - 1 && s > 0){ EXPECT(neighbors_jaccard_key((uint32_t)s, u - 1) > k0); }
	}
	EXPECT(neighbors_jaccard_key(0, 0) == 0 && neighbors_jaccard_key(5, 5) == ~0ull && neighbors_jaccard_key(0, 9) == 0);
	EXPECT(neighbors_jaccard_key(5000, 10001) > neighbors_jaccard_key(4999, 9999));
	EXPECT(neighbors_jaccard_key(0x80000000u, 1ull << 32) == 1ull << 63);
	// ---- calls
	{
		Side a(300, {7, 130, 131, 299}, rng, 5000), b(45, {33}, rng, 5000), wide(1500, {0, 700}, rng, 40);
		std::vector<uint64_t> shuffled, repeat = {5, 9, 5, 200, 5, 9};
		for(uint64_t c = 0; c < 300; ++c){ if(c != 7 && c != 130 && c != 131 && c != 299){ shuffled.push_back(c); } }
		std::shuffle(shuffled.begin(), shuffled.end(), rng);
		std::vector<uint64_t> some_b = {44, 1, 1, 20, 3};
		for(uint32_t metric : {KWAGE_NEIGHBORS_SHARED, KWAGE_NEIGHBORS_JACCARD}){
			for(int tie_mode = 0; tie_mode < 3; ++tie_mode){
				for(uint32_t k : {1u, 5u, 64u, 1024u}){
					const uint32_t min_shared = tie_mode == 0 && k == 5 ? 1500 : 0;
					for(int64_t budget : {(int64_t)1, (int64_t)128*300*4, (int64_t)256*300*4, (int64_t)1 << 28}){
						if(one_call(rng, a, nullptr, 0, nullptr, nullptr, 0, k, metric, min_shared, true, budget, 0, 5000, tie_mode)){ return 1; }
					}
					if(one_call(rng, a, shuffled.data(), shuffled.size(), &b, nullptr, 0, k, metric, min_shared, true, 128*48*4, 2, 5000, tie_mode)){ return 1; }
					if(one_call(rng, a, repeat.data(), repeat.size(), nullptr, nullptr, 0, k, metric, 0, true, 1 << 28, 0, 5000, tie_mode)){ return 1; }
					if(one_call(rng, a, repeat.data(), repeat.size(), &a, nullptr, 0, k, metric, 0, true, 1 << 28, 8, 5000, tie_mode)){ return 1; }
					if(one_call(rng, b, nullptr, 0, &a, shuffled.data(), 129, k, metric, 0, false, 1 << 28, 0, 5000, tie_mode)){ return 1; }
					if(one_call(rng, a, repeat.data(), 2, &b, some_b.data(), some_b.size(), k, metric, 0, true, 1 << 28, 0, 5000, tie_mode)){ return 1; }
				}
				// more candidates than one round of the lanes, keys that nearly all tie: the cut falls among the indices
				if(one_call(rng, b, nullptr, 0, &wide, nullptr, 0, 1024, metric, 0, false, 1 << 28, 0, 40, tie_mode)){ return 1; }
				if(one_call(rng, wide, nullptr, 0, nullptr, nullptr, 0, 7, metric, 0, true, 128*1500*4*3, 0, 40, tie_mode)){ return 1; }
			}
		}
		Side none(0, {}, rng, 1);
		if(one_call(rng, none, nullptr, 0, nullptr, nullptr, 0, 3, KWAGE_NEIGHBORS_JACCARD, 0, true, 1 << 28, 0, 1, 0)){ return 1; }
		if(one_call(rng, b, nullptr, 0, &none, nullptr, 0, 3, KWAGE_NEIGHBORS_JACCARD, 0, true, 1 << 28, 0, 1, 0)){ return 1; }
	}
	// ---- beyond 4 GiB, as pure arithmetic: 1152 entries against 2^20 candidates in one strip
	{
		const uint64_t n_a = 1152, n_b = 1ull << 20;
		EXPECT(neighbors_pitch(n_b) == n_b && neighbors_pitch(n_b + 1) == n_b + 4);
		EXPECT(neighbors_strip_entries(n_a, n_b, (int64_t)(n_a*n_b*4)) == 1152 && neighbors_strip_entries(n_a, n_b, (int64_t)(n_a*n_b*4) - 1) == 1024);
		EXPECT(neighbors_strip_entries(n_a, n_b, NEIGHBORS_STRIP_BYTES) == 128 && neighbors_strip_entries(100000, 100000, NEIGHBORS_STRIP_BYTES) == 640);
		EXPECT(neighbors_cell_offset(1024, n_b, 0)*4 == 1ull << 32 && neighbors_cell_offset(1151, n_b, n_b - 1)*4 + 4 == n_a*n_b*4);
		EXPECT(n_a*n_b*4 == 4831838208ull);
		NeighborsShape shape;
		EXPECT(neighbors_shape(WHO, n_a, n_b, 1, 256, 0, shape) == KWAGE_OK && shape.tiles.size() == 9*8192 && shape.splits == 1);
		EXPECT(neighbors_tie_bytes(n_b) == 3 && neighbors_tie_bytes(n_b*16 + 1) == 4 && neighbors_tie(3, 0) == 0xFFFFFFu && neighbors_tie(4, 5) == 0xFFFFFFFAu && neighbors_tie_bytes(256) == 1 && neighbors_tie_bytes(257) == 2);
	}
	return 0;
}

int main()
{
	if(run()){ return 1; }
	if(lists < 10000 || strips_walked < 100 || early_cuts == 0){ fprintf(stderr, "FAILED: %ld lists, %ld strips, %ld early cuts\n", lists, strips_walked, early_cuts); return 1; }
	printf("neighbors_plan.hpp under the sanitizers: %ld checks, %ld refusals, %ld lists, %ld strips: no report\n", checks, refused, lists, strips_walked);
	return 0;
}
