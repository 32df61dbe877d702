// tests/sanitize/copy_sanitize.cpp -- the host-side planning of the copy between groups (kwage_amd/csrc/copy_plan.hpp: the
// refusals, the runs, the placement, the units written, the per-unit function the kernel shares with the host) under
// -fsanitize=address,undefined.  No device: the kernel's own per-unit function runs over source and destination matrices
// whose allocations end where the matrices end, one call per (row, unit) as the kernel's lanes make them, and the
// destination is compared with a bit-by-bit restatement.
//   copy_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "copy_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, in_run = 0, walked = 0, kept = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

static bool bit(const std::vector<uint8_t> &m, uint64_t stride, uint64_t row, uint64_t c) { return (m[row*stride + c/8] >> (c%8)) & 1; }

// A source of nrows rows of `stride` bytes in an allocation of EXACTLY nrows * stride bytes: every column below the span
// random -- the invalid ones too (bits planted in pad columns: they must not travel) --, zero beyond the span.
struct Source {
	uint64_t nrows, stride, span;
	std::vector<uint8_t> bytes, valid;
	Source(uint64_t r, uint64_t s, uint64_t sp, const std::vector<uint64_t> &invalid, std::mt19937_64 &rng) : nrows(r), stride(s), span(sp), bytes(r*s, 0), valid(s, 0)
	{
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
		for(uint64_t c : invalid){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
		for(uint64_t row = 0; row < nrows; ++row){
			for(uint64_t c = 0; c < span; ++c){ if(rng() & 1){ bytes[row*stride + c/8] |= (uint8_t)(1u << (c%8)); } }
		}
	}
};

// One copy of `list` (empty: the all-columns form) into a destination of dst_stride-byte rows whose next insert lands at
// `first` (an open tail there, or -- first a multiple of 128 -- a closed one at byte first / 8): the destination holds
// random bits EVERYWHERE, below 8 * ceil(first / 8) as earlier columns and bits planted behind an open tail would, and
// above it as after a compaction of a group without valid columns, which keeps what the memory held.
static int check_copy(const Source &sx, const std::vector<uint64_t> &list, uint64_t dst_stride, uint64_t first, bool tail_open, std::mt19937_64 &rng)
{
	CopyPlan plan;
	const uint64_t next_byte = (first + 7)/8;
	EXPECT(plan_copy(list.empty() ? nullptr : list.data(), list.size(), sx.span, sx.valid.data(), next_byte, tail_open, first, dst_stride, plan) == KWAGE_OK);
	std::vector<uint64_t> cols = list;
	if(cols.empty()){ for(uint64_t c = 0; c < sx.span; ++c){ if((sx.valid[c/8] >> (c%8)) & 1){ cols.push_back(c); } } }
	const uint64_t n = cols.size();
	EXPECT(plan.first == first && plan.n == n && plan.first_unit == first/128 && plan.first_unit + plan.units == (first + n + 127)/128);
	EXPECT((plan.first_unit + plan.units)*16 <= dst_stride);
	uint64_t at = 0;
	for(size_t k = 0; k < plan.runs.size(); ++k){
		EXPECT(plan.runs[k].dst_first == at && plan.runs[k].len >= 1);
		for(uint32_t i = 0; i < plan.runs[k].len; ++i){ EXPECT(cols[at + i] == plan.runs[k].src_first + i); }
		if(k){ EXPECT(plan.runs[k].src_first != plan.runs[k - 1].src_first + plan.runs[k - 1].len); }
		at += plan.runs[k].len;
	}
	EXPECT(at == n);
	std::vector<uint8_t> dst(sx.nrows*dst_stride, 0);          // an allocation of exactly nrows * dst_stride bytes
	for(uint64_t row = 0; row < sx.nrows; ++row){
		for(uint64_t c = 0; c < 8*dst_stride; ++c){ if(rng() & 1){ dst[row*dst_stride + c/8] |= (uint8_t)(1u << (c%8)); } }
	}
	const std::vector<uint8_t> before = dst;
	const uint64_t src_bytes = sx.nrows*sx.stride;
	bool in_bounds = true;
	auto load = [&](uint64_t byte) {
		if(byte % 4 != 0 || byte + 4 > src_bytes){ in_bounds = false; return 0u; }
		uint32_t v;
		memcpy(&v, sx.bytes.data() + byte, 4);
		return v;
	};
	auto load4 = [&](uint64_t byte) {
		if(byte % 16 != 0 || byte + 16 > src_bytes){ in_bounds = false; return SaveQuad{0, 0, 0, 0}; }
		SaveQuad q;
		memcpy(&q, sx.bytes.data() + byte, 16);
		return q;
	};
	// the kernel's lanes, in shuffled order: each makes one unit and stores it once; one per row reads the destination
	std::vector<uint64_t> items(sx.nrows*plan.units);
	std::iota(items.begin(), items.end(), 0);
	std::shuffle(items.begin(), items.end(), rng);
	for(uint64_t i : items){
		const uint64_t row = i/plan.units, unit = plan.first_unit + i%plan.units;
		uint32_t w[4], keep[4];
		copy_unit_value(load, load4, plan.runs.data(), (uint32_t)plan.runs.size(), row, sx.stride, src_bytes, plan.first, plan.n, unit, w);
		if(128*unit >= first && 128*unit + 128 <= first + n){
			const uint32_t k = save_find_run(plan.runs.data(), (uint32_t)plan.runs.size(), (uint32_t)(128*unit - first));
			if(128*unit - first + 128 <= (uint64_t)plan.runs[k].dst_first + plan.runs[k].len){ ++in_run; } else { ++walked; }
		}
		else{ ++walked; }
		copy_keep_mask(plan.first, plan.n, unit, keep);
		EXPECT(row*dst_stride + 16*unit + 16 <= dst.size());
		const uint64_t last_unit = plan.first_unit + plan.units - 1;
		if((first % 128 != 0 && unit == plan.first_unit) || (((first + n - 1)/32) % 4 != 3 && unit == last_unit)){
			uint32_t old[4];
			memcpy(old, dst.data() + row*dst_stride + 16*unit, 16);
			for(int j = 0; j < 4; ++j){ w[j] |= old[j] & keep[j]; }
			++kept;
		}
		else{ EXPECT((keep[0] | keep[1] | keep[2] | keep[3]) == 0); }
		memcpy(dst.data() + row*dst_stride + 16*unit, w, 16);
	}
	EXPECT(in_bounds);
	const uint64_t written_to = ((first + n - 1)/32 + 1)*32;                                  // the end of the insert's last word
	for(uint64_t row = 0; row < sx.nrows; ++row){
		for(uint64_t c = 0; c < 8*dst_stride; ++c){
			bool want;
			if(c < first){ want = bit(before, dst_stride, row, c); }                          // kept from memory
			else if(c < first + n){ want = bit(sx.bytes, sx.stride, row, cols[c - first]); }  // the copied column
			else if(c < written_to){ want = false; }                                          // planted bits behind the tail overwritten, zero to the word's end
			else{ want = bit(before, dst_stride, row, c); }                                   // kept from memory, or not touched
			EXPECT(bit(dst, dst_stride, row, c) == want);
		}
	}
	return 0;
}

static int matrix_checks()
{
	std::mt19937_64 rng(23);
	auto range = [](uint64_t a, uint64_t b, uint64_t step = 1) { std::vector<uint64_t> v; for(uint64_t c = a; c < b; c += step){ v.push_back(c); } return v; };
	auto reversed = [](std::vector<uint64_t> v) { std::reverse(v.begin(), v.end()); return v; };
	// a full source row (the last window is the allocation's last dword) and one with pads and retired columns
	const Source full(3, 128, 1024, {}, rng), holes(3, 256, 1640, {0, 31, 32, 100, 127, 128, 129, 640, 1000, 1001, 1639}, rng);
	for(const Source *sx : {&full, &holes}){
		std::vector<uint64_t> valid;
		for(uint64_t c = 0; c < sx->span; ++c){ if((sx->valid[c/8] >> (c%8)) & 1){ valid.push_back(c); } }
		std::vector<std::vector<uint64_t>> lists;
		lists.push_back({});                                                     // the all-columns form
		lists.push_back(valid);                                                  // ascending
		lists.push_back(reversed(valid));                                        // runs of one, backwards
		{ std::vector<uint64_t> v; for(size_t i = 0; i < valid.size(); i += 2){ v.push_back(valid[i]); } lists.push_back(v); }      // runs of one
		{ std::vector<uint64_t> v = valid; std::shuffle(v.begin(), v.end(), rng); lists.push_back(v); }
		// runs that end at 32- and 128-bit boundaries of the DESTINATION (for first % 32 == 0) and of the source
		{ std::vector<uint64_t> v = range(200, 232); for(uint64_t c : range(300, 396)){ v.push_back(c); } for(uint64_t c : range(512, 640)){ v.push_back(c); } for(uint64_t c : range(33, 96)){ v.push_back(c); } lists.push_back(v); }
		for(uint64_t n : {1ull, 127ull, 128ull, 129ull}){
			lists.push_back(std::vector<uint64_t>(valid.begin() + 5, valid.begin() + 5 + n));       // one run of n
			lists.push_back(reversed(std::vector<uint64_t>(valid.end() - n, valid.end())));           // n runs of one, the source's last columns
		}
		for(const std::vector<uint64_t> &list : lists){
			for(uint64_t r : {0ull, 1ull, 31ull, 32ull, 33ull, 127ull}){
				const uint64_t n = list.empty() ? valid.size() : list.size();
				// the destination's row just wide enough, and a wide one
				for(uint64_t first : {r, 128 + r, 1024 + r}){
					const uint64_t stride = (first + n + 1023)/1024*128;
					if(check_copy(*sx, list, stride, first, true, rng)){ return 1; }
					if(first % 128 == 0 && check_copy(*sx, list, stride + 128, first, false, rng)){ return 1; }
				}
			}
		}
	}
	// a closed tail off a 16-byte boundary: the copy starts at the next one (plan_insert's rule), nothing below it is read
	{
		CopyPlan plan;
		const uint64_t one[1] = {7};
		EXPECT(plan_copy(one, 1, full.span, full.valid.data(), 9, false, 0, 128, plan) == KWAGE_OK && plan.first == 128 && plan.first_unit == 1 && plan.units == 1);
		EXPECT(plan_copy(one, 1, full.span, full.valid.data(), 9, true, 70, 128, plan) == KWAGE_OK && plan.first == 70 && plan.first_unit == 0 && plan.units == 1);
		EXPECT(plan_copy(nullptr, 0, full.span, full.valid.data(), 0, false, 0, 128, plan) == KWAGE_OK && plan.n == 1024 && plan.runs.size() == 1 && plan.units == 8);
	}
	return 0;
}

static int refusal_checks()
{
	std::mt19937_64 rng(5);
	const Source sx(1, 128, 1000, {4, 999}, rng);
	const kwage_params p{31, 3, 10, 0};
	const int ctx_a = 0, ctx_b = 0;
	const CopySide a{&ctx_a, false, p}, sparse{&ctx_a, true, p}, other{&ctx_b, false, p};
	auto group = [&](const CopySide *d, const CopySide *s, bool same, bool have_first, bool have_columns, uint64_t n, bool pending, int want) {
		++refused;
		return copy_refusal(d, s, same, have_first, have_columns, n, pending) == want && strstr(kwage_last_error(), "kwage_group_copy_columns") != nullptr;
	};
	EXPECT(group(nullptr, &a, false, true, true, 1, false, KWAGE_ERR_ARG));
	EXPECT(group(&a, nullptr, false, true, true, 1, false, KWAGE_ERR_ARG));
	EXPECT(group(&a, &a, false, false, true, 1, false, KWAGE_ERR_ARG));
	EXPECT(group(&a, &a, false, true, false, 1, false, KWAGE_ERR_ARG));            // NULL columns, n != 0
	EXPECT(group(&a, &a, false, true, true, 0, false, KWAGE_ERR_ARG));             // columns, n == 0
	EXPECT(group(&a, &a, true, true, true, 1, false, KWAGE_ERR_ARG));              // dst == src
	EXPECT(group(&a, &other, false, true, true, 1, false, KWAGE_ERR_ARG));         // another context
	EXPECT(group(&sparse, &a, false, true, true, 1, false, KWAGE_ERR_ARG));
	EXPECT(group(&a, &sparse, false, true, true, 1, false, KWAGE_ERR_ARG));
	for(int f = 0; f < 4; ++f){
		CopySide b = a;
		if(f == 0){ b.params.kmer_len = 21; } else if(f == 1){ b.params.num_hash = 2; } else if(f == 2){ b.params.log_2_filter_len = 9; } else { b.params.hash_func = 1; }
		EXPECT(group(&a, &b, false, true, true, 1, false, KWAGE_ERR_ARG));
	}
	EXPECT(group(&a, &a, false, true, true, 1, true, KWAGE_ERR_STATE));            // a search is pending
	EXPECT(group(&a, &a, true, true, true, 1, true, KWAGE_ERR_ARG));               // (the argument errors come first)
	EXPECT(copy_refusal(&a, &a, false, true, true, 1, false) == KWAGE_OK && copy_refusal(&a, &a, false, true, false, 0, false) == KWAGE_OK);
	CopyPlan plan;
	auto list = [&](const std::vector<uint64_t> &cols, uint64_t n, uint64_t next_byte, bool open, uint64_t tail, uint64_t stride) {
		++refused;
		return plan_copy(cols.empty() ? nullptr : cols.data(), n, sx.span, sx.valid.data(), next_byte, open, tail, stride, plan) == KWAGE_ERR_ARG && plan.runs.empty();
	};
	EXPECT(list({1000}, 1, 0, false, 0, 128));                                     // at the span
	EXPECT(list({1, 5000}, 2, 0, false, 0, 128));                                  // beyond it
	EXPECT(list({3, 4}, 2, 0, false, 0, 128));                                     // a retired column
	EXPECT(list({999}, 1, 0, false, 0, 128));                                      // a pad column
	EXPECT(list({7, 8, 7}, 3, 0, false, 0, 128));                                  // twice
	EXPECT(list({1}, 0x100000000ull, 0, false, 0, 128));                           // n > 2^32 - 1 (found before the list is read)
	EXPECT(list({1, 2}, 2, 128, true, 1023, 128));                                 // first + n > 8 * stride, an open tail
	EXPECT(list({1}, 1, 113, false, 0, 128));                                      // the next 16-byte boundary is the row's end
	EXPECT(list({}, 0, 0, false, 0, 64));                                          // all 998 columns into a row of 512
	{
		std::vector<uint64_t> all(16);
		std::iota(all.begin(), all.end(), 0);
		const Source none(1, 128, 16, all, rng);
		++refused;
		EXPECT(plan_copy(nullptr, 0, none.span, none.valid.data(), 0, false, 0, 128, plan) == KWAGE_ERR_ARG && strstr(kwage_last_error(), "no valid column"));
	}
	EXPECT(plan_copy(std::vector<uint64_t>{1}.data(), 1, sx.span, sx.valid.data(), 128, true, 1023, 128, plan) == KWAGE_OK && plan.first == 1023 && plan.units == 1);
	return 0;
}

static int address_checks()
{
	// row 2^32 - 1 of matrices of 12544-byte rows, source and destination: every load of a unit's value against 128-bit
	// arithmetic (the loads answer from a formula, nothing of that size is allocated), and the store's offset
	const uint64_t nrows = 1ull << 32, stride = 12544, src_bytes = nrows*stride, first = 128*3 + 33;
	std::vector<SaveRun> runs = {SaveRun{5, 0, 1000}, SaveRun{50001, 1000, 300}, SaveRun{8*stride - 700, 1300, 700}};
	const uint64_t n = 2000;
	auto word_at = [](uint64_t byte) { return (uint32_t)(byte*0x9E3779B97F4A7C15ull >> 29); };
	for(uint64_t row : std::vector<uint64_t>{0, (1ull << 31) + 3, nrows - 1}){
		const unsigned __int128 row_start = (unsigned __int128)row*stride;
		bool ok = true;
		auto load = [&](uint64_t byte) {
			if(byte % 4 || (unsigned __int128)byte < row_start || (unsigned __int128)byte + 4 > row_start + stride){ ok = false; }
			return word_at(byte);
		};
		auto load4 = [&](uint64_t byte) {
			if(byte % 16 || (unsigned __int128)byte < row_start || (unsigned __int128)byte + 16 > row_start + stride){ ok = false; }
			return SaveQuad{word_at(byte), word_at(byte + 4), word_at(byte + 8), word_at(byte + 12)};
		};
		for(uint64_t unit = first/128; unit < (first + n + 127)/128; ++unit){
			uint32_t w[4];
			copy_unit_value(load, load4, runs.data(), (uint32_t)runs.size(), row, stride, src_bytes, first, n, unit, w);
			EXPECT(ok);
			for(uint32_t b = 0; b < 128; ++b){
				const uint64_t c = 128*unit + b;
				bool want = false;
				if(c >= first && c < first + n){
					const uint64_t d = c - first, s = d < 1000 ? 5 + d : d < 1300 ? 50001 + (d - 1000) : 8*stride - 700 + (d - 1300);
					want = (word_at((uint64_t)(row_start + s/32*4)) >> (s%32)) & 1;
				}
				EXPECT((((w[b/32] >> (b%32)) & 1) != 0) == want);
			}
			EXPECT((unsigned __int128)(row*stride + 16*unit) == row_start + 16*unit && 16*unit + 16 <= stride);
		}
	}
	EXPECT((nrows - 1)*stride > (1ull << 45) && (unsigned __int128)(nrows - 1)*stride + stride == (unsigned __int128)src_bytes);
	return 0;
}

int main()
{
	if(matrix_checks() || refusal_checks() || address_checks()){ return 1; }
	if(in_run < 1000 || walked < 1000 || kept < 1000){ fprintf(stderr, "FAILED: paths taken: %ld in a run, %ld walked, %ld kept\n", in_run, walked, kept); return 1; }
	printf("copy planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
