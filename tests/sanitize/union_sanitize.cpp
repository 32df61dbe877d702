// tests/sanitize/union_sanitize.cpp -- the host-side planning of the union of columns (kwage_amd/csrc/union_plan.hpp: the
// refusals, the entries, the placement, the units written, the per-unit function the kernel shares with the host) under
// -fsanitize=address,undefined.  No device: the kernel's own per-unit function runs over source and destination matrices
// whose allocations end where the matrices end, one call per (row, unit) as the kernel's lanes make them, and the
// destination -- full of random bits beforehand -- is compared with a bit-by-bit restatement.
//   union_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "union_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, kept = 0, rounds_padded = 0, in_place = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

static bool bit(const std::vector<uint8_t> &m, uint64_t stride, uint64_t row, uint64_t c) { return (m[row*stride + c/8] >> (c%8)) & 1; }

typedef std::vector<std::vector<uint64_t>> Sets;

// A matrix of nrows rows of `stride` bytes in an allocation of EXACTLY nrows * stride bytes: every bit random -- the
// invalid columns below the span too (bits planted in pad columns: they must not travel), and everything above the span
// (what a compaction of a group without valid columns leaves).
struct Matrix {
	uint64_t nrows, stride, span;
	std::vector<uint8_t> bytes, valid;
	Matrix(uint64_t r, uint64_t s, uint64_t sp, const std::vector<uint64_t> &invalid, std::mt19937_64 &rng) : nrows(r), stride(s), span(sp), bytes(r*s, 0), valid(s, 0)
	{
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
		for(uint64_t c : invalid){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
		for(uint8_t &b : bytes){ b = (uint8_t)rng(); }
	}
};

static void flatten(const Sets &sets, std::vector<uint64_t> &columns, std::vector<uint64_t> &offsets)
{
	columns.clear();
	offsets.assign(1, 0);
	for(const auto &s : sets){
		columns.insert(columns.end(), s.begin(), s.end());
		offsets.push_back(columns.size());
	}
}

// One union of `sets` of sx's columns into `dx` (which may be sx itself: dst == src), whose next insert lands as
// next_byte / tail_open / tail say.
static int check_union(const Matrix &sx, Matrix &dx, const Sets &sets, uint64_t next_byte, bool tail_open, uint64_t tail, std::mt19937_64 &rng)
{
	const bool same = &sx == &dx;
	std::vector<uint64_t> columns, offsets;
	flatten(sets, columns, offsets);
	const uint64_t n = sets.size();
	UnionPlan plan;
	EXPECT(plan_union(columns.data(), offsets.data(), (uint32_t)n, sx.span, sx.valid.data(), same, next_byte, tail_open, tail, dx.stride, plan) == KWAGE_OK);
	const uint64_t first = tail_open && !same ? tail : (next_byte + 15)/16*16*8;
	EXPECT(plan.first == first && plan.n == n && plan.members == columns.size());
	EXPECT(plan.first_unit == first/128 && plan.first_unit + plan.units == (first + n + 127)/128 && (plan.first_unit + plan.units)*16 <= dx.stride);
	if(same){ EXPECT(first % 128 == 0 && first >= sx.span); ++in_place; }
	// the tables: per set the distinct dwords of its members, ascending, the masks exactly the members' bits
	EXPECT(plan.offsets.size() == n + 1 && plan.offsets[0] == 0 && plan.offsets[n] == plan.entries.size());
	for(uint64_t j = 0; j < n; ++j){
		std::set<uint64_t> want(sets[j].begin(), sets[j].end()), got;
		EXPECT(plan.offsets[j] < plan.offsets[j + 1]);
		for(uint32_t e = plan.offsets[j]; e < plan.offsets[j + 1]; ++e){
			const UnionEntry &en = plan.entries[e];
			EXPECT(en.mask != 0 && (e == plan.offsets[j] || plan.entries[e - 1].dword < en.dword));
			EXPECT(en.word == ((first + j) % 128)/32 && en.bit == 1u << ((first + j) % 32));
			for(uint32_t b = 0; b < 32; ++b){ if((en.mask >> b) & 1){ got.insert(32ull*en.dword + b); } }
		}
		EXPECT(got == want);
		if((plan.offsets[j + 1] - plan.offsets[j]) % UNION_LOADS){ ++rounds_padded; }
	}
	const std::vector<uint8_t> before = dx.bytes;
	const uint64_t src_bytes = sx.nrows*sx.stride;
	bool in_bounds = true, read_what_is_written = false;
	auto entry = [&](uint64_t i) {
		if(i >= plan.entries.size()){ in_bounds = false; return UnionEntry{0, 0, 0, 0}; }
		return plan.entries[i];
	};
	auto load = [&](uint64_t byte) {
		if(byte % 4 != 0 || byte + 4 > src_bytes){ in_bounds = false; return 0u; }
		// within one group: a load never touches a 16-byte unit that is stored
		if(same && byte % sx.stride >= 16*plan.first_unit){ read_what_is_written = true; }
		uint32_t v;
		memcpy(&v, (same ? before : sx.bytes).data() + byte, 4);      // (same: dx.bytes is being written; `before` is what the source held)
		return v;
	};
	// the kernel's lanes, in shuffled order: each makes one unit and stores it once
	std::vector<uint64_t> items(dx.nrows*plan.units);
	std::iota(items.begin(), items.end(), 0);
	std::shuffle(items.begin(), items.end(), rng);
	for(uint64_t i : items){
		const uint64_t row = i/plan.units, unit = plan.first_unit + i%plan.units;
		uint32_t w[4], keep[4];
		union_unit_value(entry, load, plan.offsets.data(), row, sx.stride, plan.first, plan.n, unit, w);
		copy_keep_mask(plan.first, plan.n, unit, keep);
		EXPECT(row*dx.stride + 16*unit + 16 <= dx.bytes.size());
		const uint64_t last_unit = plan.first_unit + plan.units - 1;
		if((first % 128 != 0 && unit == plan.first_unit) || (((first + n - 1)/32) % 4 != 3 && unit == last_unit)){
			uint32_t old[4];
			memcpy(old, dx.bytes.data() + row*dx.stride + 16*unit, 16);
			for(int j = 0; j < 4; ++j){ w[j] |= old[j] & keep[j]; }
			++kept;
		}
		else{ EXPECT((keep[0] | keep[1] | keep[2] | keep[3]) == 0); }
		memcpy(dx.bytes.data() + row*dx.stride + 16*unit, w, 16);
	}
	EXPECT(in_bounds && !read_what_is_written);
	const uint64_t written_to = ((first + n - 1)/32 + 1)*32;                                      // the end of the insert's last word
	for(uint64_t row = 0; row < dx.nrows; ++row){
		for(uint64_t c = 0; c < 8*dx.stride; ++c){
			bool want;
			if(c < first){ want = bit(before, dx.stride, row, c); }                               // kept from memory (within one group: the source itself)
			else if(c < first + n){
				want = false;
				for(uint64_t m : sets[c - first]){ want = want || bit(same ? before : sx.bytes, sx.stride, row, m); }      // any member's bit
			}
			else if(c < written_to){ want = false; }                                              // zero to the word's end
			else{ want = bit(before, dx.stride, row, c); }                                        // kept from memory, or not touched
			EXPECT(bit(dx.bytes, dx.stride, row, c) == want);
		}
	}
	return 0;
}

static int matrix_checks()
{
	std::mt19937_64 rng(29);
	const std::vector<uint64_t> holes = {0, 31, 32, 100, 127, 128, 129, 640, 1000, 1001, 1639};
	const Matrix full(3, 128, 1024, {}, rng), holey(3, 256, 1640, holes, rng);
	for(const Matrix *sx : {&full, &holey}){
		std::vector<uint64_t> valid;
		for(uint64_t c = 0; c < sx->span; ++c){ if((sx->valid[c/8] >> (c%8)) & 1){ valid.push_back(c); } }
		auto pick = [&](size_t k) { std::vector<uint64_t> v; for(size_t i = 0; i < k; ++i){ v.push_back(valid[rng() % valid.size()]); } return v; };
		std::vector<Sets> lists;
		lists.push_back({{valid[valid.size()/2]}});                                  // one set of one member
		lists.push_back({valid});                                                    // one set of every valid column
		{ Sets s; for(int j = 0; j < 129; ++j){ s.push_back(pick(1 + j%3)); } lists.push_back(s); }      // two units, the last holding one column
		lists.push_back({{valid[40], valid[41], valid[45]}, {valid[30], valid[70]}, {valid.front(), valid.back()}, {valid.back()}});      // one dword, adjacent dwords, the span's ends
		lists.push_back({{valid[7], valid[9], valid[7], valid[7]}});                 // a member repeated
		{ Sets s; for(int j = 0; j < 200; ++j){ s.push_back(j%2 ? std::vector<uint64_t>{valid[3]} : std::vector<uint64_t>{valid[3], pick(1)[0]}); } lists.push_back(s); }
		lists.push_back({pick(1), valid, pick(2), pick(50), pick(1), pick(17), pick(300)});               // very unequal sizes within one unit
		{ Sets s; for(uint64_t c : valid){ s.push_back({c}); } lists.push_back(s); }                      // singletons: the copy
		for(const Sets &sets : lists){
			const uint64_t n = sets.size();
			for(uint64_t r : {0ull, 1ull, 31ull, 32ull, 33ull, 127ull, 129ull}){
				// another group: an open tail at r, 128 + r; the destination's row just wide enough, and a wide one
				for(uint64_t first : {r, 1024 + r}){
					const uint64_t stride = (first + n + 1023)/1024*128;
					Matrix dx(sx->nrows, stride, 0, {}, rng);
					if(check_union(*sx, dx, sets, (first + 7)/8, true, first, rng)){ return 1; }
					Matrix wide(sx->nrows, stride + 128, 0, {}, rng);
					if(check_union(*sx, wide, sets, (first + 7)/8, false, 0, rng)){ return 1; }      // a closed tail: the next 16-byte boundary
				}
			}
			// the same group, behind an open and behind a closed tail: the row long enough for the pad and the sets
			const uint64_t stride = ((sx->span + 127)/128*128 + n + 1023)/1024*128;
			for(int open = 0; open < 2; ++open){
				Matrix g(sx->nrows, stride, sx->span, sx == &holey ? holes : std::vector<uint64_t>{}, rng);
				if(check_union(g, g, sets, (sx->span + 7)/8, open != 0, sx->span - (open ? 3 : 0), rng)){ return 1; }
			}
		}
	}
	return 0;
}

static int refusal_checks()
{
	std::mt19937_64 rng(5);
	const Matrix sx(1, 128, 1000, {4, 999}, rng);
	const kwage_params p{31, 3, 10, 0};
	const int ctx_a = 0, ctx_b = 0;
	const CopySide a{&ctx_a, false, p}, sparse{&ctx_a, true, p}, other{&ctx_b, false, p};
	const uint64_t good[3] = {0, 2, 3}, not_zero[3] = {1, 2, 3}, down[3] = {0, 2, 1}, empty[3] = {0, 2, 2};
	// every call carries every LATER fault as well: the order is the header's
	auto group = [&](const CopySide *d, const CopySide *s, bool have_columns, const uint64_t *offsets, bool have_first, uint32_t n, bool pending, int want, const char *word) {
		++refused;
		return union_refusal(d, s, have_columns, offsets, have_first, n, pending) == want && strstr(kwage_last_error(), "kwage_group_union_columns") != nullptr
		       && strstr(kwage_last_error(), word) != nullptr;
	};
	EXPECT(group(nullptr, nullptr, false, nullptr, false, 0, true, KWAGE_ERR_ARG, "NULL dst"));
	EXPECT(group(&a, nullptr, false, nullptr, false, 0, true, KWAGE_ERR_ARG, "NULL src"));
	EXPECT(group(&a, &other, false, nullptr, false, 0, true, KWAGE_ERR_ARG, "NULL columns"));
	EXPECT(group(&a, &other, true, nullptr, false, 0, true, KWAGE_ERR_ARG, "NULL set_offsets"));
	EXPECT(group(&a, &other, true, not_zero, false, 0, true, KWAGE_ERR_ARG, "NULL first_column"));
	EXPECT(group(&a, &other, true, not_zero, true, 0, true, KWAGE_ERR_ARG, "n_sets is 0"));
	EXPECT(group(&a, &other, true, not_zero, true, 2, true, KWAGE_ERR_ARG, "set_offsets[0]"));
	EXPECT(group(&a, &other, true, down, true, 2, true, KWAGE_ERR_ARG, "decreases"));
	EXPECT(group(&a, &other, true, empty, true, 2, true, KWAGE_ERR_ARG, "is empty"));
	EXPECT(group(&sparse, &other, true, good, true, 2, true, KWAGE_ERR_ARG, "different contexts"));
	CopySide b = a;
	b.params.kmer_len = 21; b.params.num_hash = 2; b.params.log_2_filter_len = 9; b.params.hash_func = 1;
	CopySide sparse_b = b;
	sparse_b.sparse = true;
	EXPECT(group(&sparse, &b, true, good, true, 2, true, KWAGE_ERR_ARG, "sparse"));
	EXPECT(group(&a, &sparse_b, true, good, true, 2, true, KWAGE_ERR_ARG, "sparse"));
	EXPECT(group(&a, &b, true, good, true, 2, true, KWAGE_ERR_ARG, "kmer_len"));
	b.params.kmer_len = 31;
	EXPECT(group(&a, &b, true, good, true, 2, true, KWAGE_ERR_ARG, "num_hash"));
	b.params.num_hash = 3;
	EXPECT(group(&a, &b, true, good, true, 2, true, KWAGE_ERR_ARG, "log_2_filter_len"));
	b.params.log_2_filter_len = 10;
	EXPECT(group(&a, &b, true, good, true, 2, true, KWAGE_ERR_ARG, "hash_func"));
	EXPECT(group(&a, &a, true, good, true, 2, true, KWAGE_ERR_STATE, "pending"));
	EXPECT(union_refusal(&a, &a, true, good, true, 2, false) == KWAGE_OK);
	UnionPlan plan;
	auto list = [&](const Sets &sets, bool same, uint64_t next_byte, bool open, uint64_t tail, uint64_t stride, const char *word) {
		std::vector<uint64_t> columns, offsets;
		flatten(sets, columns, offsets);
		++refused;
		return plan_union(columns.data(), offsets.data(), (uint32_t)sets.size(), sx.span, sx.valid.data(), same, next_byte, open, tail, stride, plan) == KWAGE_ERR_ARG
		       && plan.entries.empty() && plan.offsets.empty() && strstr(kwage_last_error(), word) != nullptr;
	};
	const Sets too_many(1025, std::vector<uint64_t>{1});
	Sets s = too_many;
	s[7] = {1, 1000, 4};
	EXPECT(list(s, false, 0, false, 0, 128, "column 1000 is at or beyond the span 1000"));      // at the span (before the pad column behind it, before the capacity)
	s[7] = {1, 5000};
	EXPECT(list(s, false, 0, false, 0, 128, "beyond the span"));
	s[7] = {3, 4};
	EXPECT(list(s, false, 0, false, 0, 128, "column 4 is a pad or retired column"));
	s[7] = {999};
	EXPECT(list(s, true, 0, false, 0, 128, "column 999 is a pad or retired column"));
	++refused;
	EXPECT(union_count_refusal(0x100000000ull) == KWAGE_ERR_ARG && strstr(kwage_last_error(), "do not fit") && union_count_refusal(0xFFFFFFFFull) == KWAGE_OK);
	EXPECT(list(too_many, false, 0, false, 0, 128, "capacity exceeded"));
	EXPECT(list({{1}, {2}}, false, 128, true, 1023, 128, "capacity exceeded"));                 // first + n > 8 * stride, an open tail
	EXPECT(list({{1}}, false, 113, false, 0, 128, "capacity exceeded"));                        // the next 16-byte boundary is the row's end
	EXPECT(list({{1}}, true, 125, true, 1000, 128, "capacity exceeded"));                       // within one group the open tail's room does not count
	{
		std::vector<uint64_t> columns, offsets;
		flatten({{1}}, columns, offsets);
		EXPECT(plan_union(columns.data(), offsets.data(), 1, sx.span, sx.valid.data(), false, 125, true, 1000, 128, plan) == KWAGE_OK && plan.first == 1000 && plan.units == 1);
		EXPECT(plan_union(columns.data(), offsets.data(), 1, sx.span, sx.valid.data(), true, 112, true, 890, 128, plan) == KWAGE_OK && plan.first == 896 && plan.first_unit == 7);
	}
	return 0;
}

static int address_checks()
{
	// row 2^32 - 1 of matrices of 12544-byte rows, source and destination: every load of a unit's value against 128-bit
	// arithmetic (the loads answer from a formula, nothing of that size is allocated), and the store's offset
	const uint64_t nrows = 1ull << 32, stride = 12544, first = 128*3 + 33;
	const Sets sets = {{5}, {8*stride - 1, 0, 50001}, {31, 32, 63, 64}, {8*stride - 32, 8*stride - 33}};
	std::vector<uint64_t> columns, offsets;
	flatten(sets, columns, offsets);
	Sets many;
	for(uint64_t j = 0; j < 300; ++j){ many.push_back(sets[j % sets.size()]); }
	flatten(many, columns, offsets);
	const std::vector<uint8_t> valid(stride, 0xFF);
	UnionPlan plan;
	EXPECT(plan_union(columns.data(), offsets.data(), (uint32_t)many.size(), 8*stride, valid.data(), false, (first + 7)/8, true, first, stride, plan) == KWAGE_OK);
	auto word_at = [](uint64_t byte) { return (uint32_t)(byte*0x9E3779B97F4A7C15ull >> 29); };
	auto entry = [&](uint64_t i) { return plan.entries[i]; };
	for(uint64_t row : std::vector<uint64_t>{0, (1ull << 31) + 3, nrows - 1}){
		const unsigned __int128 row_start = (unsigned __int128)row*stride;
		bool ok = true;
		auto load = [&](uint64_t byte) {
			if(byte % 4 || (unsigned __int128)byte < row_start || (unsigned __int128)byte + 4 > row_start + stride){ ok = false; }
			return word_at(byte);
		};
		for(uint64_t unit = plan.first_unit; unit < plan.first_unit + plan.units; ++unit){
			uint32_t w[4];
			union_unit_value(entry, load, plan.offsets.data(), row, stride, plan.first, plan.n, unit, w);
			EXPECT(ok);
			for(uint32_t b = 0; b < 128; ++b){
				const uint64_t c = 128*unit + b;
				bool want = false;
				if(c >= first && c < first + many.size()){
					for(uint64_t m : many[c - first]){ want = want || ((word_at((uint64_t)(row_start + m/32*4)) >> (m%32)) & 1); }
				}
				EXPECT((((w[b/32] >> (b%32)) & 1) != 0) == want);
			}
			EXPECT((unsigned __int128)(row*stride + 16*unit) == row_start + 16*unit && 16*unit + 16 <= stride);
		}
	}
	EXPECT((nrows - 1)*stride > (1ull << 45) && (unsigned __int128)(nrows - 1)*stride + stride == (unsigned __int128)nrows*stride);
	return 0;
}

int main()
{
	if(matrix_checks() || refusal_checks() || address_checks()){ return 1; }
	if(kept < 1000 || rounds_padded < 1000 || in_place < 10){ fprintf(stderr, "FAILED: paths taken: %ld kept, %ld padded rounds, %ld in place\n", kept, rounds_padded, in_place); return 1; }
	printf("union planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
