// tests/sanitize/export_sanitize.cpp -- the host-side planning of the export (kwage_amd/csrc/export_plan.hpp: the runs a
// column list folds into, duplicates included, the rows of a staged chunk, the grid, and the host restatement of what the
// kernel stores as one dword of one filter) under -fsanitize=address,undefined.  No device: the functions take plain values.
//   export_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "export_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, in_run = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)
static const char *WHO = "kwage_group_export_filters";

// A small matrix: nrows rows of `stride` bytes in an allocation of EXACTLY nrows * stride bytes (the sanitizer sees any
// window that reads past it), columns [0, span) of which `valid` are real.
struct Matrix {
	uint64_t nrows, stride, span;
	std::vector<uint8_t> bytes, valid;
	Matrix(uint64_t r, uint64_t s, uint64_t sp, std::mt19937_64 &rng) : nrows(r), stride(s), span(sp), bytes(r*s), valid(s, 0)
	{
		for(auto &b : bytes){ b = (uint8_t)rng(); }
		for(uint64_t c = 0; c < span; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
	}
	bool bit(uint64_t row, uint64_t c) const { return (bytes[row*stride + c/8] >> (c%8)) & 1; }
	void retire(uint64_t c) { valid[c/8] &= (uint8_t)~(1u << (c%8)); }
};

// One list over one chunk of rows [row_base, row_base + chunk_rows): the plan against a per-filter restatement, every
// dword of every filter through export_dword against a naive bit-by-bit transpose, and the kernel's load phase (the unit
// inside one run, else the walk) against the same bits.
static int check_list(const Matrix &m, const std::vector<uint64_t> &cols, uint64_t row_base, uint64_t chunk_rows)
{
	std::vector<SaveRun> runs;
	EXPECT(plan_export(WHO, cols.data(), cols.size(), m.span, m.valid.data(), runs) == KWAGE_OK);
	const uint32_t n = (uint32_t)cols.size();
	uint64_t at = 0;
	for(size_t k = 0; k < runs.size(); ++k){
		EXPECT(runs[k].dst_first == at && runs[k].len >= 1);
		for(uint32_t i = 0; i < runs[k].len; ++i){ EXPECT(cols[at + i] == runs[k].src_first + i); }
		if(k){ EXPECT(runs[k].src_first != runs[k - 1].src_first + runs[k - 1].len); }      // (else the two were one run)
		at += runs[k].len;
	}
	EXPECT(at == n);

	const uint64_t matrix_bytes = m.nrows*m.stride;
	bool in_bounds = true;
	auto load = [&](uint64_t byte) {
		if(byte % 4 != 0 || byte + 4 > matrix_bytes){ in_bounds = false; return 0u; }
		uint32_t v;
		memcpy(&v, m.bytes.data() + byte, 4);
		return v;
	};
	auto load4 = [&](uint64_t byte) {
		if(byte % 16 != 0 || byte + 16 > matrix_bytes){ in_bounds = false; return SaveQuad{0, 0, 0, 0}; }
		SaveQuad q;
		memcpy(&q, m.bytes.data() + byte, 16);
		return q;
	};
	const uint64_t dwords = (chunk_rows + 31)/32;
	for(uint32_t f = 0; f < n; ++f){
		for(uint64_t j = 0; j < dwords; ++j){
			uint32_t want = 0;
			for(uint32_t b = 0; b < 32 && 32*j + b < chunk_rows; ++b){ want |= (uint32_t)m.bit(row_base + 32*j + b, cols[f]) << b; }
			EXPECT(export_dword(load, runs.data(), (uint32_t)runs.size(), n, row_base, chunk_rows, m.stride, matrix_bytes, f, j) == want);
		}
	}
	// the load phase of export_filters_kernel: 16-byte units of 128 listed filters
	for(uint64_t r = 0; r < chunk_rows; ++r){
		const uint64_t row = row_base + r;
		for(uint64_t d0 = 0; d0 < n; d0 += 128){
			uint32_t k = save_find_run(runs.data(), (uint32_t)runs.size(), (uint32_t)d0);
			const SaveRun first = runs[k];
			uint32_t w[4];
			if(d0 + 128 <= (uint64_t)first.dst_first + first.len){
				save_unit_in_run(load, load4, row, m.stride, first.src_first + ((uint32_t)d0 - first.dst_first), w);
				++in_run;
			}
			else{
				for(int j = 0; j < 4; ++j){
					const uint64_t b = d0 + 32u*j;
					w[j] = b < n ? save_word(load, runs.data(), &k, row, m.stride, matrix_bytes, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + 32, n)) : 0u;
				}
			}
			for(uint32_t i = 0; i < 128; ++i){
				const bool want = d0 + i < n && m.bit(row, cols[d0 + i]);
				EXPECT((((w[i/32] >> (i%32)) & 1) != 0) == want);
			}
		}
	}
	EXPECT(in_bounds);
	return 0;
}

static int list_checks()
{
	std::mt19937_64 rng(23);
	Matrix m(40, 128, 1000, rng);                    // span 1000 of a capacity of 1024: the last windows end at the allocation
	for(uint64_t c : {300ull, 331ull, 332ull, 363ull, 500ull, 999ull}){ m.retire(c); }
	std::vector<uint64_t> real;
	for(uint64_t c = 0; c < m.span; ++c){ if((m.valid[c/8] >> (c%8)) & 1){ real.push_back(c); } }
	std::vector<std::vector<uint64_t>> lists;
	lists.push_back(real);                                                   // ascending, with holes
	lists.push_back(std::vector<uint64_t>(real.rbegin(), real.rend()));      // reversed
	{ std::vector<uint64_t> a; for(size_t i = 0; i < real.size(); i += 3){ a.push_back(real[i]); } lists.push_back(a); }      // scattered
	lists.push_back({7, 7, 7});                                              // duplicates: a column three times ...
	lists.push_back({5, 6, 7, 5, 6, 7, 8, 9, 5});                            // ... runs that repeat ...
	{ std::vector<uint64_t> a; for(int k = 0; k < 3; ++k){ for(uint64_t c = 100; c < 260; ++c){ a.push_back(c); } } lists.push_back(a); }     // ... and long ones
	lists.push_back({998});                                                  // the last valid column alone
	for(const auto &l : lists){ if(check_list(m, l, 0, 40)){ return 1; } }
	if(check_list(m, real, 8, 24)){ return 1; }                              // a chunk in the middle, and one that ends in a byte
	if(check_list(m, lists[2], 32, 8)){ return 1; }

	// a full matrix: the span IS the capacity.  Every first column 0 .. 127, run lengths around the 32-filter group and the
	// 128-filter unit, alone and behind three scattered filters (the run then starts off a word of the output)
	Matrix full(33, 128, 1024, rng);
	for(uint64_t first = 0; first < 128; ++first){
		for(uint64_t len : {1ull, 31ull, 32ull, 33ull, 127ull, 128ull, 129ull}){
			std::vector<uint64_t> l(len);
			std::iota(l.begin(), l.end(), first);
			if(check_list(full, l, 0, 33)){ return 1; }
			if(first % 9 == 0){
				std::vector<uint64_t> p = {1023, 0, 511};
				p.insert(p.end(), l.begin(), l.end());
				if(check_list(full, p, 0, 33)){ return 1; }
			}
		}
	}
	{ std::vector<uint64_t> tail(417); std::iota(tail.begin(), tail.end(), 607); if(check_list(full, tail, 0, 33)){ return 1; } }      // up to the last column of the row

	// refusals: nothing planned
	std::vector<SaveRun> runs;
	auto refuse = [&](const std::vector<uint64_t> &l) {
		++refused;
		return plan_export(WHO, l.data(), l.size(), m.span, m.valid.data(), runs) == KWAGE_ERR_ARG && runs.empty() && strstr(kwage_last_error(), WHO) != nullptr;
	};
	EXPECT(refuse({}));                               // n == 0
	EXPECT(refuse({5, 1000}));                        // at the span
	EXPECT(refuse({5, 1023}));                        // beyond it
	EXPECT(refuse({1ull << 40}));
	EXPECT(refuse({5, 300}));                         // retired
	EXPECT(refuse({999}));
	EXPECT(refuse({5, 5, 363}));
	++refused;
	EXPECT(plan_export(WHO, real.data(), 1ull << 32, m.span, m.valid.data(), runs) == KWAGE_ERR_ARG && runs.empty());      // more than a run table counts (refused before the list is read)
	return 0;
}

static int address_checks()
{
	// a row offset beyond 2^32 (arithmetic only): the last rows of a 2^23-row matrix of 12544-byte rows.  export_dword asks
	// for exactly the dwords a 128-bit restatement names, all inside the matrix.
	const uint64_t nrows = 1ull << 23, stride = 12544, matrix_bytes = nrows*stride;
	const std::vector<uint64_t> cols = {8*stride - 1, 0, 33, 34, 35, 8*stride - 32};
	std::vector<uint8_t> valid(stride, 0xFF);
	std::vector<SaveRun> runs;
	EXPECT(plan_export(WHO, cols.data(), cols.size(), 8*stride, valid.data(), runs) == KWAGE_OK && runs.size() == 4);
	for(uint64_t j : std::vector<uint64_t>{0, (1ull << 18) - 1}){          // first and last dword of a filter
		for(uint32_t f = 0; f < cols.size(); ++f){
			bool ok = true;
			uint64_t asked = 0;
			auto load = [&](uint64_t byte) {
				++asked;
				if(byte % 4 != 0 || byte + 4 > matrix_bytes){ ok = false; }
				// the value says which (row, dword of the row) was read: bit = (row + dword) & 1
				const uint64_t row = byte/stride, dw = (byte % stride)/4;
				return ((row + dw) & 1) ? 0xFFFFFFFFu : 0u;
			};
			const uint32_t got = export_dword(load, runs.data(), (uint32_t)runs.size(), (uint32_t)cols.size(), 0, nrows, stride, matrix_bytes, f, j);
			uint32_t want = 0;
			for(uint32_t b = 0; b < 32; ++b){
				const unsigned __int128 byte = (unsigned __int128)(32*j + b)*stride + cols[f]/32*4;
				EXPECT(byte + 4 <= matrix_bytes);
				want |= (uint32_t)((((uint64_t)(byte/stride) + (uint64_t)(byte % stride)/4) & 1)) << b;
			}
			EXPECT(ok && asked > 0 && got == want);
		}
	}
	EXPECT(save_window(nrows - 1, stride, cols[0]).byte == matrix_bytes - 4 && matrix_bytes > (1ull << 36));
	return 0;
}

static int chunk_checks()
{
	// every chunk plan: whole bytes of a filter, the pieces fit the staging (down to one byte each), the chunks cover a
	// filter exactly once, the device stride holds a piece and keeps dwords aligned
	for(uint64_t nrows : std::vector<uint64_t>{1, 2, 4, 8, 32, 64, 1024, 8192, 1ull << 23, 1ull << 32}){
		for(uint64_t n : std::vector<uint64_t>{1, 31, 70, 1024, 8192}){
			for(uint64_t staging : std::vector<uint64_t>{0, 1, n - 1, n, n + 1, 2*n, 63*n, 64*n, 65*n, 4096, 100000, 1ull << 30, ~0ull}){
				const ExportChunks c = plan_export_chunks(staging, n, nrows);
				EXPECT(c.filter_bytes == std::max<uint64_t>(1, nrows/8));
				EXPECT(c.chunk_bytes >= 1 && c.chunk_bytes <= c.filter_bytes);
				const uint64_t bound = staging ? staging : (64ull << 20);
				EXPECT(c.chunk_bytes == 1 || c.chunk_bytes <= bound/n);
				EXPECT(c.chunk_bytes == c.filter_bytes || c.chunk_bytes < 64 || c.chunk_bytes % 64 == 0);
				EXPECT(c.rows == std::min(8*c.chunk_bytes, nrows) && (c.rows % 8 == 0 || c.rows == nrows));
				EXPECT(c.chunks == (c.filter_bytes + c.chunk_bytes - 1)/c.chunk_bytes && (c.chunks - 1)*c.chunk_bytes < c.filter_bytes);
				EXPECT(c.dev_stride >= c.chunk_bytes && c.dev_stride % 4 == 0 && c.dev_stride < c.chunk_bytes + 512);
				EXPECT(c.chunk_bytes < 256 || (c.dev_stride/256) % 2 == 1);
			}
		}
	}
	ExportChunks c = plan_export_chunks(70, 70, 8192);                     // one byte of every filter per chunk
	EXPECT(c.chunk_bytes == 1 && c.rows == 8 && c.chunks == 1024 && c.dev_stride == 4);
	c = plan_export_chunks(4096, 70, 8192);
	EXPECT(c.chunk_bytes == 58 && c.rows == 464 && c.chunks == 18);
	c = plan_export_chunks(0, 1024, 1ull << 23);                           // 1024 filters of a MiB each: 64 KiB of each per chunk
	EXPECT(c.chunk_bytes == 65536 && c.chunks == 16 && c.dev_stride == 65536 + 256);
	c = plan_export_chunks(0, 3, 4);                                       // L = 2: one byte, all four rows
	EXPECT(c.filter_bytes == 1 && c.chunk_bytes == 1 && c.rows == 4 && c.chunks == 1);

	// the grid: a workgroup per tile, row tiles first
	ExportGrid g = export_grid(8192, 2049, 512, 1024);
	EXPECT(g.ok && g.tiles_x == 16 && g.tiles_f == 3);
	g = export_grid(1, 1, 512, 1024);
	EXPECT(g.ok && g.tiles_x == 1 && g.tiles_f == 1);
	g = export_grid(1ull << 32, 1024, 512, 1024);
	EXPECT(g.ok && g.tiles_x == (1ull << 23) && g.tiles_f == 1);
	g = export_grid(1ull << 32, 1ull << 20, 512, 1024);                    // more tiles than one launch takes
	EXPECT(!g.ok);
	return 0;
}

int main()
{
	if(list_checks() || address_checks() || chunk_checks()){ return 1; }
	if(in_run < 150){ fprintf(stderr, "FAILED: only %ld units took the in-run path\n", in_run); return 1; }
	printf("export planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
