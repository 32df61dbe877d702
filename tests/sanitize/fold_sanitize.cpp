// tests/sanitize/fold_sanitize.cpp -- the host-side planning of the fold (kwage_amd/csrc/fold_plan.hpp: the refusals, the
// units, items, chunks and grid, the loads per item and pass, the byte counts, the item arithmetic the kernel shares with
// the host) under -fsanitize=address,undefined.  No device: the kernel's schedule runs on host matrices whose allocations
// end exactly where the matrices end -- whole chunks with all loads of a pass made before any is used, other chunks item by
// item through fold_item_value -- and the result is compared with a bit-by-bit OR.
//   fold_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fold_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, whole_chunks = 0, cut_chunks = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

// The kernel on the host: src of EXACTLY 2^L * stride bytes, dst of exactly 2^L2 * stride bytes (zero, as allocated).
static int emulate(const std::vector<uint8_t> &src, std::vector<uint8_t> &dst, const FoldPlan &plan, uint64_t stride, int ncu)
{
	bool in_bounds = true;
	auto load4 = [&](uint64_t byte) {
		FoldQuad q = {0, 0, 0, 0};
		if(byte % 16 != 0 || byte + 16 > src.size()){ in_bounds = false; return q; }
		memcpy(&q, src.data() + byte, 16);
		return q;
	};
	std::vector<uint8_t> written(dst.size()/16, 0);
	auto store = [&](uint64_t byte, const FoldQuad &q) {
		if(byte % 16 != 0 || byte + 16 > dst.size() || written[byte/16]){ in_bounds = false; return; }
		written[byte/16] = 1;
		memcpy(dst.data() + byte, &q, 16);
	};
	const uint32_t loads = 1u << plan.J, ipl = plan.items_per_lane;
	EXPECT(loads*ipl == FOLD_LOADS_IN_FLIGHT && (uint64_t)loads*plan.passes == (1ull << plan.f));
	EXPECT(plan.grid <= (uint64_t)ncu*8 && plan.grid <= plan.chunks && (plan.grid > 0) == (plan.items > 0));
	for(uint32_t wg = 0; wg < plan.grid; ++wg){
		for(uint64_t chunk = wg; chunk < plan.chunks; chunk += plan.grid){
			const bool whole = fold_chunk_item(chunk, ipl, ipl - 1, FOLD_THREADS - 1) < plan.items;
			++(whole ? whole_chunks : cut_chunks);
			for(uint32_t lane = 0; lane < FOLD_THREADS; ++lane){
				if(whole){
					std::vector<uint64_t> byte(ipl);
					std::vector<FoldQuad> acc(ipl, FoldQuad{0, 0, 0, 0}), v((size_t)ipl*loads);
					for(uint32_t i = 0; i < ipl; ++i){ byte[i] = fold_item(fold_chunk_item(chunk, ipl, i, lane), plan.units_per_row, stride).byte; }
					uint64_t at = 0;
					for(uint32_t p = 0; p < plan.passes; ++p){
						for(uint32_t i = 0; i < ipl; ++i){ for(uint32_t j = 0; j < loads; ++j){ v[i*loads + j] = load4(byte[i] + at + j*plan.src_step); } }
						for(uint32_t i = 0; i < ipl; ++i){
							for(uint32_t j = 0; j < loads; ++j){
								const FoldQuad &q = v[i*loads + j];
								acc[i].x |= q.x; acc[i].y |= q.y; acc[i].z |= q.z; acc[i].w |= q.w;
							}
						}
						at += (uint64_t)loads*plan.src_step;
					}
					for(uint32_t i = 0; i < ipl; ++i){ store(byte[i], acc[i]); }
				}
				else{
					for(uint32_t i = 0; i < ipl; ++i){
						const uint64_t item = fold_chunk_item(chunk, ipl, i, lane);
						if(item >= plan.items){ continue; }
						const uint64_t byte = fold_item(item, plan.units_per_row, stride).byte;
						store(byte, fold_item_value(load4, byte, plan.src_step, (uint64_t)plan.passes*loads));
					}
				}
			}
		}
	}
	EXPECT(in_bounds);
	// every unit of every destination row below units_per_row exactly once, nothing else
	for(uint64_t u = 0; u < written.size(); ++u){ EXPECT(written[u] == ((u % (stride/16)) < plan.units_per_row ? 1 : 0)); }
	return 0;
}

static int check_shape(uint32_t L, uint32_t L2, uint64_t stride, uint64_t row_bytes, int ncu, std::mt19937_64 &rng)
{
	const uint64_t nrows = 1ull << L, dst_rows = 1ull << L2;
	std::vector<uint8_t> src(nrows*stride, 0), dst(dst_rows*stride, 0);      // allocations of exactly the matrices' bytes
	// random bits at 1/8 on the whole stride: what lies beyond 16 * units_per_row must not reach the destination
	for(uint8_t &b : src){ b = (uint8_t)(rng() & rng() & rng() & 0xFF); }
	const FoldPlan plan = plan_fold(L, L2, row_bytes, stride, ncu);
	EXPECT(plan.f == L - L2 && plan.J == std::min<uint32_t>(plan.f, 3) && plan.units_per_row == (row_bytes + 15)/16 && plan.units_per_row*16 <= stride);
	EXPECT(plan.dst_rows == dst_rows && plan.items == dst_rows*plan.units_per_row && plan.src_step == dst_rows*stride);
	EXPECT(plan.bytes_written == 16*plan.items && plan.bytes_read == plan.bytes_written << plan.f);
	EXPECT(plan.chunks*FOLD_THREADS*plan.items_per_lane >= plan.items && (plan.chunks == 0 || (plan.chunks - 1)*FOLD_THREADS*plan.items_per_lane < plan.items));
	if(emulate(src, dst, plan, stride, ncu)){ return 1; }
	// bit by bit: the OR of the 2^f source rows; zero from 16 * units_per_row to the stride
	for(uint64_t r = 0; r < dst_rows; ++r){
		for(uint64_t c = 0; c < 8*stride; ++c){
			bool want = false;
			if(c < 128*plan.units_per_row){
				for(uint64_t j = 0; j < (1ull << plan.f); ++j){ want = want || ((src[(r + j*dst_rows)*stride + c/8] >> (c%8)) & 1); }
			}
			EXPECT((((dst[r*stride + c/8] >> (c%8)) & 1) != 0) == want);
		}
	}
	// the host restatement of single items against the same OR, bytewise
	for(int t = 0; t < 8 && plan.items; ++t){
		const uint64_t item = rng() % plan.items;
		const FoldItem it = fold_item(item, plan.units_per_row, stride);
		EXPECT(it.row == item/plan.units_per_row && it.unit == item % plan.units_per_row && it.byte == it.row*stride + 16*it.unit);
		uint8_t want[16] = {0};
		for(uint64_t j = 0; j < (1ull << plan.f); ++j){ for(int b = 0; b < 16; ++b){ want[b] |= src[(it.row + j*dst_rows)*stride + 16*it.unit + b]; } }
		const FoldQuad q = fold_item_value([&](uint64_t byte) { FoldQuad x; memcpy(&x, src.data() + byte, 16); return x; }, it.byte, plan.src_step, 1ull << plan.f);
		EXPECT(memcmp(&q, want, 16) == 0);
	}
	return 0;
}

static int matrix_checks()
{
	std::mt19937_64 rng(23);
	struct Shape { uint32_t L, L2; uint64_t stride, row_bytes; int ncu; };
	const Shape shapes[] = {
		{1, 0, 128, 1, 4}, {3, 2, 128, 15, 4}, {3, 0, 128, 16, 4}, {8, 7, 128, 17, 1}, {8, 6, 128, 128, 1}, {8, 5, 256, 129, 1},
		{8, 4, 1152, 1025, 1}, {8, 0, 1152, 1025, 2}, {10, 9, 128, 127, 1}, {10, 8, 256, 130, 1}, {9, 6, 128, 33, 1},      // several chunks per workgroup
		{6, 3, 384, 257, 256}, {7, 5, 128, 0, 4},                                                                            // an empty span: nothing launched
		{11, 10, 128, 128, 1}, {10, 8, 256, 256, 3}, {10, 7, 256, 250, 1},                                                   // whole chunks only, for each J
		{12, 1, 128, 100, 4},                                                                                             // 2^8 passes
	};
	for(const Shape &s : shapes){ if(check_shape(s.L, s.L2, s.stride, s.row_bytes, s.ncu, rng)){ return 1; } }
	return 0;
}

static int refusal_checks()
{
	auto refuse = [&](int want, bool src, bool out, bool sparse, uint32_t L, uint32_t L2, bool pending) {
		++refused;
		return fold_refusal(src, out, sparse, L, L2, pending) == want;
	};
	EXPECT(refuse(KWAGE_ERR_ARG, false, true, false, 0, 0, false));
	EXPECT(refuse(KWAGE_ERR_ARG, true, false, false, 8, 7, false));
	EXPECT(refuse(KWAGE_ERR_ARG, true, true, true, 8, 7, false));
	EXPECT(refuse(KWAGE_ERR_ARG, true, true, false, 8, 8, false));
	EXPECT(refuse(KWAGE_ERR_ARG, true, true, false, 8, 9, false));
	EXPECT(refuse(KWAGE_ERR_ARG, true, true, false, 0, 0, false));
	EXPECT(refuse(KWAGE_ERR_STATE, true, true, false, 8, 7, true));
	EXPECT(refuse(KWAGE_ERR_ARG, true, true, false, 8, 8, true));          // (the argument is refused first)
	EXPECT(fold_refusal(true, true, false, 8, 7, false) == KWAGE_OK && fold_refusal(true, true, false, 1, 0, false) == KWAGE_OK);
	return 0;
}

static int address_checks()
{
	// destination row 2^32 - 1 of 12544-byte rows (784 units), folded from 2^33 rows: the item numbers, the unit's offset
	// and its second source's offset against 128-bit arithmetic; nothing of that size is allocated
	const uint64_t stride = 12544, row_bytes = 12537;
	const FoldPlan plan = plan_fold(33, 32, row_bytes, stride, 256);
	EXPECT(plan.units_per_row == 784 && plan.J == 1 && plan.items_per_lane == 4 && plan.passes == 1 && plan.grid == 2048);
	EXPECT((unsigned __int128)plan.items == (unsigned __int128)784 << 32 && (unsigned __int128)plan.src_step == (unsigned __int128)stride << 32);
	EXPECT((unsigned __int128)plan.bytes_read == ((unsigned __int128)784 << 32)*32 && plan.bytes_written == plan.bytes_read/2);
	const uint64_t row = (1ull << 32) - 1;
	for(uint64_t u = 0; u < 784; u += 1 + u % 7){
		const uint64_t item = row*784 + u;
		EXPECT((item >> 32) != 0);
		const FoldItem it = fold_item(item, plan.units_per_row, stride);
		EXPECT(it.row == row && it.unit == u);
		EXPECT((unsigned __int128)it.byte == (unsigned __int128)row*stride + 16*u);
		EXPECT((unsigned __int128)(it.byte + plan.src_step) == ((unsigned __int128)row + ((unsigned __int128)1 << 32))*stride + 16*u);
		EXPECT((unsigned __int128)it.byte + plan.src_step + 16 <= ((unsigned __int128)stride << 33));
		// the item is the lane's of exactly one chunk
		const uint64_t per = (uint64_t)FOLD_THREADS*plan.items_per_lane, chunk = item/per, in = item % per;
		EXPECT(fold_chunk_item(chunk, plan.items_per_lane, (uint32_t)(in/FOLD_THREADS), (uint32_t)(in % FOLD_THREADS)) == item);
	}
	// the 32-bit division's range ends where the item number gets its 33rd bit
	for(uint64_t item : {0xFFFFFFFFull, 0x100000000ull, 0x100000001ull}){
		for(uint64_t U : {1ull, 3ull, 784ull, 0x7FFFFFFFull}){
			const FoldItem it = fold_item(item, U, 128*((16*U + 127)/128));
			EXPECT(it.row == item/U && it.unit == item % U);
		}
	}
	return 0;
}

int main()
{
	if(refusal_checks() || matrix_checks() || address_checks()){ return 1; }
	if(whole_chunks < 20 || cut_chunks < 8){ fprintf(stderr, "FAILED: paths taken: %ld whole chunks, %ld cut\n", whole_chunks, cut_chunks); return 1; }
	printf("fold planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
