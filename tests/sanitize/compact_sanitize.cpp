// tests/sanitize/compact_sanitize.cpp -- the host-side planning of the compaction (kwage_amd/csrc/compact_plan.hpp: the
// runs the survivors fold into, the units rewritten, the schedule of a row, the per-unit function the kernel shares with
// the host) under -fsanitize=address,undefined.  No device: the kernel's own per-unit function runs IN PLACE on host
// matrices whose allocation ends where the matrix ends, in the kernel's schedule -- all units of a segment made, then all
// stored -- with the units of a segment visited forwards, backwards and shuffled, the rows in shuffled order.
//   compact_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "compact_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, in_run = 0, walked = 0, zeroed = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

// nrows rows of `stride` bytes in an allocation of EXACTLY nrows * stride bytes; columns [0, span) random where valid,
// zero elsewhere (retire clears a column's bits; pads are zero), and zero beyond the span.
struct Matrix {
	uint64_t nrows, stride, span;
	std::vector<uint8_t> bytes, valid;
	Matrix(uint64_t r, uint64_t s, uint64_t sp, const std::vector<uint64_t> &invalid, std::mt19937_64 &rng) : nrows(r), stride(s), span(sp), bytes(r*s, 0), valid(s, 0)
	{
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
		for(uint64_t c : invalid){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
		for(uint64_t row = 0; row < nrows; ++row){
			for(uint64_t c = 0; c < span; ++c){
				if(compact_is_valid(valid.data(), c) && (rng() & 1)){ bytes[row*stride + c/8] |= (uint8_t)(1u << (c%8)); }
			}
		}
	}
};

enum Order { FORWARDS, BACKWARDS, SHUFFLED };

// The kernel on the host, in place.
static int emulate(std::vector<uint8_t> &mem, uint64_t nrows, uint64_t stride, const CompactPlan &plan, uint32_t threads, Order order, std::mt19937_64 &rng)
{
	const uint64_t matrix_bytes = nrows*stride;
	if(plan.first_unit == plan.end_unit){ return 0; }      // (nothing is launched)
	bool in_bounds = true;
	uint64_t floor_byte = 0;     // no load of the unit being made may lie below the unit's own first byte
	auto load = [&](uint64_t byte) {
		if(byte % 4 != 0 || byte + 4 > matrix_bytes || byte < floor_byte){ in_bounds = false; return 0u; }
		uint32_t v;
		memcpy(&v, mem.data() + byte, 4);
		return v;
	};
	auto load4 = [&](uint64_t byte) {
		if(byte % 16 != 0 || byte + 16 > matrix_bytes || byte < floor_byte){ in_bounds = false; return SaveQuad{0, 0, 0, 0}; }
		SaveQuad q;
		memcpy(&q, mem.data() + byte, 16);
		return q;
	};
	const CompactSchedule s = compact_schedule(plan.first_unit, plan.end_unit, threads);
	EXPECT(s.lanes >= 8 && s.lanes <= threads && s.lanes*s.rows_per_wg == threads && (s.lanes & (s.lanes - 1)) == 0);
	EXPECT(s.segments*s.lanes >= plan.end_unit - plan.first_unit && (s.segments - 1)*s.lanes < plan.end_unit - plan.first_unit);
	std::vector<uint64_t> rows(nrows);
	std::iota(rows.begin(), rows.end(), 0);
	std::shuffle(rows.begin(), rows.end(), rng);
	std::vector<uint32_t> lanes(s.lanes);
	struct Made { uint64_t u; uint32_t w[4]; };
	std::vector<Made> made;
	for(uint64_t row : rows){
		for(uint64_t seg = 0; seg < s.segments; ++seg){
			std::iota(lanes.begin(), lanes.end(), 0u);
			if(order == BACKWARDS){ std::reverse(lanes.begin(), lanes.end()); }
			if(order == SHUFFLED){ std::shuffle(lanes.begin(), lanes.end(), rng); }
			made.clear();
			for(uint32_t lane : lanes){
				const uint64_t u = compact_unit_of(plan.first_unit, seg, s.lanes, lane);
				if(u >= plan.end_unit){ continue; }
				Made md;
				md.u = u;
				floor_byte = row*stride + 16*u;
				if(128*u >= plan.m){ ++zeroed; }
				else{
					const uint32_t k = save_find_run(plan.runs.data(), (uint32_t)plan.runs.size(), (uint32_t)(128*u));
					if(128*u + 128 <= (uint64_t)plan.runs[k].dst_first + plan.runs[k].len){ ++in_run; } else { ++walked; }
				}
				compact_unit(load, load4, plan.runs.data(), (uint32_t)plan.runs.size(), (uint32_t)plan.m, row, stride, matrix_bytes, u, md.w);
				made.push_back(md);
			}
			// (the barrier) -- and the stores, in the other direction
			if(order != SHUFFLED){ std::reverse(made.begin(), made.end()); } else { std::shuffle(made.begin(), made.end(), rng); }
			for(const Made &md : made){
				EXPECT(16*md.u + 16 <= stride);
				memcpy(mem.data() + row*stride + 16*md.u, md.w, 16);
			}
		}
	}
	EXPECT(in_bounds);
	return 0;
}

// One matrix: the plan against a per-column restatement, then the emulated kernel in every order against a bit-by-bit
// restatement made from a copy.
static int check_matrix(const Matrix &mx, bool tail_open, uint64_t tail, uint32_t threads, std::mt19937_64 &rng)
{
	CompactPlan plan;
	EXPECT(plan_compact(mx.valid.data(), mx.span, tail_open, tail, false, 0, plan) == KWAGE_OK);
	std::vector<uint64_t> survivors;
	for(uint64_t c = 0; c < mx.span; ++c){ if(compact_is_valid(mx.valid.data(), c)){ survivors.push_back(c); } }
	const uint64_t m = survivors.size();
	EXPECT(plan.m == m && plan.span_before == mx.span);
	uint64_t at = 0;
	for(size_t k = 0; k < plan.runs.size(); ++k){
		EXPECT(plan.runs[k].dst_first == at && plan.runs[k].len >= 1 && plan.runs[k].src_first >= plan.runs[k].dst_first);
		for(uint32_t i = 0; i < plan.runs[k].len; ++i){ EXPECT(survivors[at + i] == plan.runs[k].src_first + i); }
		if(k){ EXPECT(plan.runs[k].src_first != plan.runs[k - 1].src_first + plan.runs[k - 1].len); }
		at += plan.runs[k].len;
	}
	EXPECT(at == m);
	uint64_t p = mx.span;
	for(uint64_t c = 0; c < mx.span; ++c){ if(!compact_is_valid(mx.valid.data(), c)){ p = c; break; } }
	if(plan.nothing_to_close || m == 0){ EXPECT(plan.first_unit == plan.end_unit); }
	else{ EXPECT(plan.first_unit == p/128 && plan.end_unit == (mx.span + 127)/128 && plan.end_unit*16 <= mx.stride); }
	EXPECT(plan.nothing_to_close == (p >= (tail_open ? tail : mx.span)));
	// the map and the mask
	std::vector<uint64_t> map(mx.span + 1, 77);
	compact_fill_map(mx.valid.data(), mx.span, map.data());
	uint64_t rank = 0;
	for(uint64_t c = 0; c < mx.span; ++c){
		if(compact_is_valid(mx.valid.data(), c)){ EXPECT(map[c] == rank); ++rank; } else { EXPECT(map[c] == 0xFFFFFFFFFFFFFFFFull); }
	}
	EXPECT(map[mx.span] == 77);
	std::vector<uint8_t> mask = mx.valid;
	compact_valid_mask(mask.data(), mx.span/8, m);
	for(uint64_t c = 0; c < 8*mx.stride; ++c){ EXPECT(compact_is_valid(mask.data(), c) == (c < m)); }
	// the matrix, in every order
	for(Order order : {FORWARDS, BACKWARDS, SHUFFLED}){
		std::vector<uint8_t> mem = mx.bytes;          // an allocation of exactly nrows * stride bytes
		if(emulate(mem, mx.nrows, mx.stride, plan, threads, order, rng)){ return 1; }
		for(uint64_t row = 0; row < mx.nrows; ++row){
			for(uint64_t d = 0; d < 8*mx.stride; ++d){
				const bool got = (mem[row*mx.stride + d/8] >> (d%8)) & 1;
				bool want;
				if(d < m){ const uint64_t c = survivors[d]; want = (mx.bytes[row*mx.stride + c/8] >> (c%8)) & 1; }
				else{ want = false; }                 // zero from m to the old span; beyond it the matrix was zero
				EXPECT(got == want);
			}
		}
	}
	return 0;
}

static int matrix_checks()
{
	std::mt19937_64 rng(17);
	auto range = [](uint64_t a, uint64_t b, uint64_t step = 1) { std::vector<uint64_t> v; for(uint64_t c = a; c < b; c += step){ v.push_back(c); } return v; };
	auto join = [](std::vector<uint64_t> a, const std::vector<uint64_t> &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
	struct Shape { uint64_t nrows, stride, span; std::vector<uint64_t> invalid; uint32_t threads; };
	std::vector<Shape> shapes;
	// rows of 1 KiB (64 units) with workgroups of 16 threads: four segments and more, the shift of one bit
	for(uint64_t span : {8192ull, 8184ull, 8072ull, 1032ull}){
		shapes.push_back({3, 1024, span, {0}, 16});
		shapes.push_back({3, 1024, span, range(0, 700), 16});                    // sources more than a segment (16 units) ahead
		shapes.push_back({2, 1024, span, {900}, 16});                            // an identity prefix
		shapes.push_back({2, 1024, span, range(200, 712, 2), 16});               // runs of one
		shapes.push_back({2, 1024, span, join(range(128, 256), range(512, 1024)), 16});      // whole units
		shapes.push_back({2, 1024, span, {31, 32, 127, 128, 129}, 16});
		shapes.push_back({2, 1024, span, range(span - 200, span), 16});          // nothing moves
		shapes.push_back({2, 1024, span, range(0, span), 16});                   // m == 0
		shapes.push_back({2, 1024, span, {}, 16});                               // nothing to close
		shapes.push_back({2, 1024, span, range(5, 6), 256});                     // fewer units than threads: one segment
	}
	// rows of 128 and 256 bytes: several rows to a workgroup; alignment pads only
	shapes.push_back({70, 128, 560, join(join(range(70, 128), range(129, 256)), range(556, 560)), 256});
	shapes.push_back({40, 256, 2048, join(range(3, 4), range(1000, 1100)), 256});
	shapes.push_back({33, 128, 1024, {1023}, 256});
	shapes.push_back({33, 128, 1024, {0}, 256});                                 // the full row: the last window is the allocation's last dword
	for(int round = 0; round < 40; ++round){                                     // random holes
		const uint64_t span = 8*(1 + rng() % 1024);
		std::vector<uint64_t> inv;
		const uint64_t density = 1 + rng() % 200;
		for(uint64_t c = 0; c < span; ++c){ if(rng() % density == 0){ inv.push_back(c); } }
		shapes.push_back({2, 1024, span, inv, (uint32_t)(8u << (rng() % 6))});
	}
	for(const Shape &sh : shapes){
		Matrix mx(sh.nrows, sh.stride, sh.span, sh.invalid, rng);
		if(check_matrix(mx, false, 0, sh.threads, rng)){ return 1; }
	}
	// an open tail: the columns between the tail and the span are no hole
	{
		Matrix mx(2, 1024, 1000, range(997, 1000), rng);
		CompactPlan plan;
		EXPECT(plan_compact(mx.valid.data(), mx.span, true, 997, false, 0, plan) == KWAGE_OK && plan.nothing_to_close && plan.m == 997 && plan.first_unit == plan.end_unit);
		if(check_matrix(mx, true, 997, 16, rng)){ return 1; }
		Matrix my(2, 1024, 1000, join(range(10, 11), range(997, 1000)), rng);
		if(check_matrix(my, true, 997, 16, rng)){ return 1; }
	}
	// refusals: nothing planned
	{
		Matrix mx(1, 128, 1000, {4}, rng);
		CompactPlan plan;
		auto refuse = [&](uint64_t capacity) { ++refused; return plan_compact(mx.valid.data(), mx.span, false, 0, true, capacity, plan) == KWAGE_ERR_ARG && plan.runs.empty(); };
		EXPECT(refuse(0));
		EXPECT(refuse(1));
		EXPECT(refuse(999));
		EXPECT(plan_compact(mx.valid.data(), mx.span, false, 0, true, 1000, plan) == KWAGE_OK && plan.runs.size() == 2);
		EXPECT(plan_compact(mx.valid.data(), mx.span, false, 0, false, 0, plan) == KWAGE_OK);      // (no map: capacity does not count)
	}
	return 0;
}

static int address_checks()
{
	// the last row of a 2^23-row matrix of 12544-byte rows (784 units): every load and the store of its units against
	// 128-bit arithmetic; the loads answer from a formula, nothing of that size is allocated
	const uint64_t nrows = 1ull << 23, stride = 12544, matrix_bytes = nrows*stride, span = 8*stride;
	std::vector<uint8_t> valid(stride, 0xFF);
	valid[0] = 0xFE;                                                             // column 0 retired: one run, every unit shifted by a bit
	for(uint64_t c : {50000ull, 50001ull, 99999ull}){ valid[c/8] &= (uint8_t)~(1u << (c%8)); }
	CompactPlan plan;
	EXPECT(plan_compact(valid.data(), span, false, 0, false, 0, plan) == KWAGE_OK && plan.m == span - 4 && plan.runs.size() == 3);
	EXPECT(plan.first_unit == 0 && plan.end_unit == 784);
	const CompactSchedule s = compact_schedule(plan.first_unit, plan.end_unit, 256);
	EXPECT(s.lanes == 256 && s.rows_per_wg == 1 && s.segments == 4);
	auto word_at = [](uint64_t byte) { return (uint32_t)(byte*0x9E3779B97F4A7C15ull >> 29); };
	for(uint64_t row : std::vector<uint64_t>{0, (1ull << 19) + 3, nrows - 1}){
		const unsigned __int128 row_start = (unsigned __int128)row*stride;
		bool ok = true;
		unsigned __int128 floor_byte = 0;
		auto load = [&](uint64_t byte) {
			if(byte % 4 || (unsigned __int128)byte < floor_byte || (unsigned __int128)byte + 4 > row_start + stride){ ok = false; }
			return word_at(byte);
		};
		auto load4 = [&](uint64_t byte) {
			if(byte % 16 || (unsigned __int128)byte < floor_byte || (unsigned __int128)byte + 16 > row_start + stride){ ok = false; }
			return SaveQuad{word_at(byte), word_at(byte + 4), word_at(byte + 8), word_at(byte + 12)};
		};
		for(uint64_t seg = 0; seg < s.segments; ++seg){
			for(uint32_t lane = 0; lane < s.lanes; lane += 1 + lane % 5){
				const uint64_t u = compact_unit_of(plan.first_unit, seg, s.lanes, lane);
				if(u >= plan.end_unit){ continue; }
				floor_byte = row_start + 16*u;
				uint32_t w[4];
				compact_unit(load, load4, plan.runs.data(), (uint32_t)plan.runs.size(), (uint32_t)plan.m, row, stride, matrix_bytes, u, w);
				EXPECT(ok);
				for(int j = 0; j < 4; ++j){                                      // destination bits against the formula, column by column
					for(uint32_t b = 0; b < 32; b += 7){
						const uint64_t d = 128*u + 32u*j + b;
						bool want = false;
						if(d < plan.m){
							const uint64_t c = d + 1 + (d + 1 >= 50000 ? 2 : 0) + (d + 3 >= 99999 ? 1 : 0);
							const unsigned __int128 byte = row_start + c/32*4;
							want = (word_at((uint64_t)byte) >> (c%32)) & 1;
						}
						EXPECT((((w[j] >> b) & 1) != 0) == want);
					}
				}
			}
		}
	}
	EXPECT((nrows - 1)*stride > (1ull << 36));
	return 0;
}

int main()
{
	if(matrix_checks() || address_checks()){ return 1; }
	if(in_run < 1000 || walked < 200 || zeroed < 50){ fprintf(stderr, "FAILED: paths taken: %ld in a run, %ld walked, %ld zero\n", in_run, walked, zeroed); return 1; }
	printf("compact planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
