// tests/sanitize/save_sanitize.cpp -- the host-side planning of the save (kwage_amd/csrc/save_plan.hpp: the runs a column
// list folds into, the address function and the window rule the kernel shares with the host, the rows of a staged chunk)
// under -fsanitize=address,undefined.  No device: the functions take plain values.
//   save_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "save_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, in_run = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

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

// The kernel on the host: every 16-byte unit of every output row through save_find_run + save_unit_in_run / save_word, as
// extract_columns_kernel does it, the loads through the matrix's own bytes with a bound check of the window.
static int emulate(const Matrix &m, const std::vector<SaveRun> &runs, uint32_t n, std::vector<uint8_t> &out)
{
	const uint64_t out_slice = ((uint64_t)n + 7)/8, units = (out_slice + 15)/16, matrix_bytes = m.nrows*m.stride;
	out.assign(m.nrows*out_slice, 0xAA);
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
	for(uint64_t row = 0; row < m.nrows; ++row){
		for(uint64_t u = 0; u < units; ++u){
			const uint32_t d0 = (uint32_t)(128*u);
			uint32_t k = save_find_run(runs.data(), (uint32_t)runs.size(), d0);
			const SaveRun first = runs[k];
			uint32_t w[4];
			if((uint64_t)d0 + 128 <= (uint64_t)first.dst_first + first.len){
				save_unit_in_run(load, load4, row, m.stride, first.src_first + (d0 - first.dst_first), w);
				++in_run;
			}
			else{
				for(int j = 0; j < 4; ++j){
					const uint64_t b = (uint64_t)d0 + 32u*j;
					w[j] = b < n ? save_word(load, runs.data(), &k, row, m.stride, matrix_bytes, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + 32, n)) : 0u;
				}
			}
			const uint64_t nb = std::min<uint64_t>(16, out_slice - 16*u);
			for(uint64_t j = 0; j < nb; ++j){ out[row*out_slice + 16*u + j] = (uint8_t)(w[j/4] >> (8*(j%4))); }
		}
	}
	EXPECT(in_bounds);
	return 0;
}

// One list: the plan against a per-bit restatement, then every destination bit of the emulated kernel.
static int check_list(const Matrix &m, const std::vector<uint64_t> &cols)
{
	std::vector<SaveRun> runs;
	EXPECT(plan_save(cols.data(), cols.size(), m.span, m.valid.data(), runs) == KWAGE_OK);
	// the runs cover [0, n) in order without gaps, are maximal, and say where every destination column comes from
	const uint32_t n = (uint32_t)cols.size();
	uint64_t at = 0;
	for(size_t k = 0; k < runs.size(); ++k){
		EXPECT(runs[k].dst_first == at && runs[k].len >= 1);
		for(uint32_t i = 0; i < runs[k].len; ++i){ EXPECT(cols[at + i] == runs[k].src_first + i); }
		if(k){ EXPECT(runs[k].src_first != runs[k - 1].src_first + runs[k - 1].len); }      // (else the two were one run)
		at += runs[k].len;
	}
	EXPECT(at == n);
	for(uint32_t d = 0; d < n; d += 1 + d/7){
		const uint32_t k = save_find_run(runs.data(), (uint32_t)runs.size(), d);
		EXPECT(runs[k].dst_first <= d && d - runs[k].dst_first < runs[k].len);
	}
	std::vector<uint8_t> out;
	if(emulate(m, runs, n, out)){ return 1; }
	const uint64_t out_slice = ((uint64_t)n + 7)/8;
	for(uint64_t row = 0; row < m.nrows; ++row){
		for(uint64_t d = 0; d < 8*out_slice; ++d){
			const bool want = d < n && m.bit(row, cols[d]);                  // pad bits of the last byte: zero
			EXPECT((((out[row*out_slice + d/8] >> (d%8)) & 1) != 0) == want);
		}
	}
	return 0;
}

static int list_checks()
{
	std::mt19937_64 rng(16);
	Matrix m(5, 128, 1000, rng);                     // span 1000 of a capacity of 1024: the last windows end at the allocation
	for(uint64_t c : {0ull, 31ull, 32ull, 33ull, 63ull, 64ull, 99ull, 500ull, 999ull}){ m.retire(c); }
	std::vector<uint64_t> real;
	for(uint64_t c = 0; c < m.span; ++c){ if((m.valid[c/8] >> (c%8)) & 1){ real.push_back(c); } }
	std::vector<std::vector<uint64_t>> lists;
	lists.push_back(real);                                                   // ascending, with holes
	lists.push_back(std::vector<uint64_t>(real.rbegin(), real.rend()));      // reversed
	{ std::vector<uint64_t> p = real; std::shuffle(p.begin(), p.end(), rng); lists.push_back(p); }      // permuted
	{ std::vector<uint64_t> a; for(size_t i = 0; i < real.size(); i += 2){ a.push_back(real[i]); } lists.push_back(a); }      // alternating
	for(uint64_t c : {1ull, 30ull, 34ull, 998ull}){ lists.push_back({c}); }  // single columns
	for(uint64_t first : {1ull, 5ull, 65ull, 100ull, 101ull, 127ull}){       // one run at every kind of offset, every length around the units
		for(uint64_t len : {1ull, 7ull, 8ull, 9ull, 31ull, 32ull, 33ull, 127ull, 128ull, 129ull, 255ull, 256ull, 260ull}){
			std::vector<uint64_t> l;
			for(uint64_t c = first; l.size() < len && c < 500; ++c){ if((m.valid[c/8] >> (c%8)) & 1){ l.push_back(c); } }
			lists.push_back(l);
		}
	}
	{ std::vector<uint64_t> tail; for(uint64_t c = 960; c < 999; ++c){ tail.push_back(c); } lists.push_back(tail); }      // the last dword of a row
	for(int round = 0; round < 60; ++round){                                 // random subsets in random order
		std::vector<uint64_t> p = real;
		std::shuffle(p.begin(), p.end(), rng);
		p.resize(1 + rng() % 300);
		if(round % 2){ std::sort(p.begin(), p.end()); }
		lists.push_back(p);
	}
	for(const auto &l : lists){ if(check_list(m, l)){ return 1; } }
	// a full matrix: the span IS the capacity, the last column's window is the allocation's last dword
	Matrix full(3, 128, 1024, rng);
	std::vector<uint64_t> all(1024);
	std::iota(all.begin(), all.end(), 0);
	if(check_list(full, all)){ return 1; }
	std::vector<uint64_t> last(all.begin() + 1001, all.end());
	if(check_list(full, last)){ return 1; }
	// whole units inside one run, from every kind of start: a 16-byte boundary (one 16-byte load), a dword boundary that is
	// none, either with a bit offset (the fifth dword), and up to the last column of the row
	for(uint64_t first : {128ull, 160ull, 133ull, 167ull, 255ull, 512ull, 607ull}){
		std::vector<uint64_t> l(all.begin() + (long)first, all.begin() + (long)std::min<uint64_t>(first + 417, 1024));
		if(check_list(full, l)){ return 1; }
	}

	// refusals: nothing planned
	std::vector<SaveRun> runs;
	auto refuse = [&](const std::vector<uint64_t> &l) { ++refused; return plan_save(l.data(), l.size(), m.span, m.valid.data(), runs) == KWAGE_ERR_ARG && runs.empty(); };
	EXPECT(refuse({}));                               // n == 0
	EXPECT(refuse({5, 1000}));                        // at the span
	EXPECT(refuse({5, 1023}));                        // beyond it
	EXPECT(refuse({1ull << 40}));
	EXPECT(refuse({5, 31}));                          // retired
	EXPECT(refuse({999}));
	EXPECT(refuse({5, 6, 5}));                        // twice
	EXPECT(refuse({7, 7}));
	++refused;
	EXPECT(plan_save(real.data(), 1ull << 32, m.span, m.valid.data(), runs) == KWAGE_ERR_ARG && runs.empty());      // more than num_filter holds (refused before the list is read)
	return 0;
}

static int address_checks()
{
	// exact beyond 2^32: the last row of a 2^23-row matrix of 12544-byte rows, against 128-bit arithmetic
	const uint64_t nrows = 1ull << 23, stride = 12544, matrix_bytes = nrows*stride;
	for(uint64_t row : std::vector<uint64_t>{0, 1, (1ull << 19) + 3, nrows - 1}){
		for(uint64_t c : std::vector<uint64_t>{0, 1, 31, 32, 33, 2047, 2048, 8*stride - 33, 8*stride - 32, 8*stride - 1}){
			const SaveWindow w = save_window(row, stride, c);
			const unsigned __int128 want = (unsigned __int128)row*stride + c/32*4;
			EXPECT((unsigned __int128)w.byte == want && w.shift == c % 32 && w.byte % 4 == 0);
			EXPECT(w.byte + 4 <= matrix_bytes);                              // never beyond nrows * stride
			EXPECT(8*(w.byte - row*stride) + w.shift == c);
		}
	}
	EXPECT(save_window(nrows - 1, stride, 0).byte > (1ull << 32) && save_window(nrows - 1, stride, 8*stride - 1).byte == matrix_bytes - 4);
	// the window rule at that row: pieces of every length at every shift, the second dword asked for only where the
	// piece reaches into it and never beyond the matrix
	std::mt19937_64 rng(3);
	for(uint64_t row : std::vector<uint64_t>{nrows - 1, nrows - 2}){
		for(uint64_t c = 8*stride - 96; c < 8*stride; ++c){
			for(uint32_t cnt = 1; cnt <= 32 && c + cnt <= 8*stride; ++cnt){
				const uint32_t lo_v = (uint32_t)rng(), hi_v = (uint32_t)rng();
				const uint64_t base = row*stride + c/32*4;
				int loads = 0;
				bool ok = true;
				auto load = [&](uint64_t byte) {
					++loads;
					if(byte + 4 > matrix_bytes || (byte != base && byte != base + 4)){ ok = false; }
					return byte == base ? lo_v : hi_v;
				};
				const uint32_t got = save_piece(load, row, stride, matrix_bytes, c, cnt);
				const uint64_t both = ((uint64_t)lo_v | ((uint64_t)hi_v << 32)) >> (c % 32);
				EXPECT(ok && got == (uint32_t)(both & (cnt == 32 ? 0xFFFFFFFFull : ((1ull << cnt) - 1))));
				EXPECT(loads == (c % 32 + cnt > 32 ? 2 : 1));
			}
		}
	}
	return 0;
}

static int chunk_checks()
{
	// 100 columns: out_slice 13; 1024 rows
	SaveChunks c = plan_chunks(0, 100, 1024);
	EXPECT(c.out_slice == 13 && c.rows == 1024 && c.chunks == 1);                        // 0 = 64 MiB: the whole body
	c = plan_chunks(1, 100, 1024);
	EXPECT(c.rows == 1 && c.chunks == 1024);                                              // less than a row: one row per chunk
	c = plan_chunks(12, 100, 1024);
	EXPECT(c.rows == 1 && c.chunks == 1024);
	c = plan_chunks(13, 100, 1024);
	EXPECT(c.rows == 1 && c.chunks == 1024);
	for(uint64_t k : {2ull, 3ull, 256ull, 341ull, 512ull, 1023ull, 1024ull}){             // exactly k rows, and a byte less
		c = plan_chunks(13*k, 100, 1024);
		EXPECT(c.rows == k && c.chunks == (1024 + k - 1)/k);
		c = plan_chunks(13*k - 1, 100, 1024);
		EXPECT(c.rows == k - 1 && c.chunks == (1024 + k - 2)/(k - 1));
	}
	c = plan_chunks(13*1024 + 1, 100, 1024);
	EXPECT(c.rows == 1024 && c.chunks == 1);
	c = plan_chunks(~0ull, 100, 1024);                                                    // larger than the whole body
	EXPECT(c.rows == 1024 && c.chunks == 1);
	c = plan_chunks(0, 2048, 1ull << 23);                                                 // the reference's file: 2 GiB of body in 64 MiB chunks
	EXPECT(c.out_slice == 256 && c.rows == (1ull << 18) && c.chunks == 32);
	c = plan_chunks(0, 0xFFFFFFFFull, 1ull << 32);
	EXPECT(c.out_slice == (1ull << 29) && c.rows == 1 && c.chunks == (1ull << 32));
	c = plan_chunks(5, 1, 1);                                                             // one column of a one-row filter
	EXPECT(c.out_slice == 1 && c.rows == 1 && c.chunks == 1);
	return 0;
}

int main()
{
	if(list_checks() || address_checks() || chunk_checks()){ return 1; }
	if(in_run < 150){ fprintf(stderr, "FAILED: only %ld units took the in-run path\n", in_run); return 1; }
	printf("save planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
