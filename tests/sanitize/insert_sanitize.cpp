// tests/sanitize/insert_sanitize.cpp -- the host-side planning of the live insert (kwage_amd/csrc/insert_plan.hpp: the
// reservation rule, the span a launch covers, the retire word and mask folding) and the `.bloom` validation
// (bloom_files.hpp) under -fsanitize=address,undefined.  No device: the functions take plain values.
//   insert_sanitize <golden dir> <scratch dir>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "bloom_files.hpp"
#include "insert_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while(0)

// A model group: what insert.hip and loader.hip do to next_byte / the tail / the valid mask, on a bit vector.
struct Model {
	uint64_t stride, next_byte = 0, tail = 0, num_columns = 0;
	bool open = false;
	std::vector<uint8_t> valid;
	explicit Model(uint64_t s) : stride(s), valid(s, 0) {}
	int insert(uint64_t n, uint64_t *first)
	{
		int rc = plan_insert(next_byte, open, tail, stride, n, first);
		if(rc){ return rc; }
		for(uint64_t c = *first; c < *first + n; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }
		tail = *first + n; open = true; next_byte = (tail + 7)/8; num_columns += n;
		return 0;
	}
	int block(uint64_t n)          // group_reserve_columns
	{
		const uint64_t start = (next_byte + 15)/16*16, width = (n + 7)/8;
		if(n == 0 || start + width > stride){ return -1; }
		for(uint64_t c = 0; c < n; ++c){ valid[start + c/8] |= (uint8_t)(1u << (c%8)); }
		next_byte = start + width; num_columns += n; open = false;
		return 0;
	}
};

static int plan_checks()
{
	uint64_t first = 99;
	// the first insert starts at column 0, the next at the very next column: 1000 one at a time == one call of 1000
	Model a(256), b(256);
	for(int i = 0; i < 1000; ++i){ EXPECT(a.insert(1, &first) == 0 && first == (uint64_t)i); }
	EXPECT(b.insert(1000, &first) == 0 && first == 0);
	EXPECT(a.next_byte == 125 && b.next_byte == 125 && a.valid == b.valid && a.tail == b.tail);
	// a block closes the tail; the insert behind it starts on a 16-byte boundary
	EXPECT(a.block(13) == 0 && a.next_byte == 128 + 2 && !a.open);
	EXPECT(a.insert(3, &first) == 0 && first == 8*144 && a.next_byte == 145 && a.open);
	EXPECT(a.insert(6, &first) == 0 && first == 8*144 + 3 && a.next_byte == 146);
	// capacity: exactly full is fine, one more is refused and changes nothing
	Model c(128);
	EXPECT(c.insert(1023, &first) == 0 && c.insert(1, &first) == 0 && first == 1023 && c.next_byte == 128);
	const Model before = c;
	first = 77;
	EXPECT(c.insert(1, &first) == KWAGE_ERR_ARG && first == 77); ++refused;
	EXPECT(c.insert(0, &first) == KWAGE_ERR_ARG); ++refused;
	EXPECT(c.next_byte == before.next_byte && c.tail == before.tail && c.valid == before.valid);
	Model d(128);
	EXPECT(d.block(900) == 0);            // next_byte 113: the boundary behind it is the stride itself
	EXPECT(d.insert(1, &first) == KWAGE_ERR_ARG); ++refused;
	EXPECT(plan_insert(0, false, 0, 128, 1025, &first) == KWAGE_ERR_ARG); ++refused;
	EXPECT(plan_insert(0, true, 5, 1ull << 40, 0xFFFFFFFFull, &first) == 0 && first == 5);

	// the span of a launch, for every bit offset and a few lengths
	for(uint64_t f = 0; f < 300; ++f){
		for(uint64_t n : {1ull, 7ull, 31ull, 32ull, 33ull, 127ull, 128ull, 129ull, 1024ull, 5000ull}){
			const InsertSpan s = insert_span(f, n);
			EXPECT(s.word_base % 4 == 0 && s.word_base <= s.word_first && s.word_first - s.word_base < 4);
			EXPECT(32*s.word_first + s.keep_bits == f && 32*s.word_base + s.shift == f && s.shift < 128);
			EXPECT(32*s.word_last <= f + n - 1 && f + n - 1 < 32*s.word_last + 32);
		}
	}
	return 0;
}

static int retire_checks()
{
	std::mt19937_64 rng(5);
	std::vector<uint8_t> valid(64, 0);
	for(uint64_t c = 0; c < 300; ++c){ valid[c/8] |= (uint8_t)(1u << (c%8)); }      // columns 0 .. 299 real, span 512
	std::vector<RetirePair> pairs;
	uint64_t distinct = 0;
	const uint64_t two[] = {37, 33, 37, 299, 0, 31, 32};
	EXPECT(plan_retire(valid.data(), 512, two, 7, pairs, &distinct) == 0 && distinct == 6 && pairs.size() == 3);
	EXPECT(pairs[0].word == 0 && pairs[0].mask == 0x80000001u && pairs[1].word == 1 && pairs[1].mask == ((1u << 5) | (1u << 1) | 1u));
	EXPECT(pairs[2].word == 9 && pairs[2].mask == (1u << 11));
	const uint64_t pad[] = {5, 300}, beyond[] = {5, 512};
	EXPECT(plan_retire(valid.data(), 512, pad, 2, pairs, &distinct) == KWAGE_ERR_ARG && pairs.empty() && distinct == 0); ++refused;
	EXPECT(plan_retire(valid.data(), 512, beyond, 2, pairs, &distinct) == KWAGE_ERR_ARG); ++refused;
	EXPECT(plan_retire(valid.data(), 512, nullptr, 0, pairs, &distinct) == 0 && pairs.empty());
	for(int round = 0; round < 2000; ++round){
		std::vector<uint64_t> cols(1 + rng() % 40);
		std::vector<uint8_t> want(64, 0);
		for(auto &c : cols){ c = rng() % 300; want[c/8] |= (uint8_t)(1u << (c%8)); }
		EXPECT(plan_retire(valid.data(), 512, cols.data(), cols.size(), pairs, &distinct) == 0);
		std::vector<uint8_t> got(64, 0);
		uint64_t bits = 0;
		for(size_t i = 0; i < pairs.size(); ++i){
			EXPECT(pairs[i].mask != 0 && (i == 0 || pairs[i].word > pairs[i - 1].word) && pairs[i].word < 16);
			for(int k = 0; k < 4; ++k){ got[4*pairs[i].word + k] |= (uint8_t)(pairs[i].mask >> (8*k)); }
			bits += (uint64_t)__builtin_popcount(pairs[i].mask);
		}
		EXPECT(got == want && bits == distinct);
	}
	return 0;
}

static bool write_file(const std::string &path, const std::vector<unsigned char> &b)
{
	FILE *f = fopen(path.c_str(), "wb");
	if(!f){ return false; }
	const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
	return fclose(f) == 0 && ok;
}

static int bloom_checks(const std::string &golden, const std::string &scratch)
{
	// the fixtures' own parameters come from their first file
	const std::string dir = golden + "/basic/bloom/";
	std::vector<std::string> names;
	for(int i = 0; i < 8; ++i){ char b[32]; snprintf(b, sizeof(b), "f%06d.bloom", i); names.push_back(dir + b); }
	FILE *f = fopen(names[0].c_str(), "rb");
	EXPECT(f != nullptr);
	std::vector<unsigned char> raw(1 << 22);
	raw.resize(fread(raw.data(), 1, raw.size(), f));
	fclose(f);
	EXPECT(raw.size() > 21);
	kwage_params p{rd32(raw.data() + 1), rd32(raw.data() + 9), rd32(raw.data() + 5), (int32_t)rd32(raw.data() + 13)};
	const uint64_t filter_bytes = ((1ull << p.log_2_filter_len) + 7)/8;
	std::vector<const char*> paths;
	for(auto &n : names){ paths.push_back(n.c_str()); }
	std::vector<BloomFile> files;
	EXPECT(open_bloom_files("test", paths.data(), (uint32_t)paths.size(), &p, files) == 0 && files.size() == paths.size());
	for(auto &bf : files){ EXPECT(bf.map && bf.size - bf.bits_off >= filter_bytes); bf.close_file(); }

	// damaged copies of the first file, each as the LAST of three: all are checked before anything would be written
	auto refuse = [&](const std::vector<unsigned char> &bytes, int want) -> int {
		const std::string bad = scratch + "/bad.bloom";
		if(!write_file(bad, bytes)){ return 1; }
		const char *three[] = {names[1].c_str(), names[2].c_str(), bad.c_str()};
		std::vector<BloomFile> fs;
		const int rc = open_bloom_files("test", three, 3, &p, fs);
		++refused;
		for(auto &bf : fs){ if(bf.map || bf.fd >= 0){ return 1; } }      // everything closed again
		return rc == want ? 0 : 1;
	};
	std::vector<unsigned char> b = raw;
	b[raw.size() - 1] ^= 0x10;
	EXPECT(refuse(b, KWAGE_ERR_FORMAT) == 0);                       // a flipped payload bit: CRC32
	b = raw; b[9] ^= 1;
	EXPECT(refuse(b, KWAGE_ERR_ARG) == 0);                          // another num_hash
	b = raw; b[1] ^= 2;
	EXPECT(refuse(b, KWAGE_ERR_ARG) == 0);                          // another kmer_len
	b = raw; b[0] = 0;
	EXPECT(refuse(b, KWAGE_ERR_FORMAT) == 0);                       // incomplete
	for(size_t cut : {(size_t)0, (size_t)1, (size_t)20, (size_t)21, (size_t)40, raw.size() - filter_bytes, raw.size() - 1}){
		b.assign(raw.begin(), raw.begin() + (long)cut);
		EXPECT(refuse(b, KWAGE_ERR_FORMAT) == 0);                   // truncated at every kind of boundary
	}
	const char *missing[] = {names[0].c_str(), "/nonexistent/x.bloom"};
	EXPECT(open_bloom_files("test", missing, 2, &p, files) == KWAGE_ERR_IO); ++refused;
	const char *null_name[] = {names[0].c_str(), nullptr};
	EXPECT(open_bloom_files("test", null_name, 2, &p, files) == KWAGE_ERR_ARG); ++refused;
	std::mt19937_64 rng(9);
	for(int round = 0; round < 200; ++round){                      // random damage: any status, no report
		b = raw;
		for(int k = 0; k < 3; ++k){ b[rng() % std::min<size_t>(b.size(), 200)] = (unsigned char)rng(); }
		if(rng() % 4 == 0){ b.resize(rng() % b.size()); }
		if(!write_file(scratch + "/bad.bloom", b)){ return 1; }
		const std::string bad = scratch + "/bad.bloom";
		const char *one[] = {bad.c_str()};
		std::vector<BloomFile> fs;
		if(open_bloom_files("test", one, 1, &p, fs) != 0){ ++refused; }
		for(auto &bf : fs){ bf.close_file(); }
		++checks;
	}
	return 0;
}

int main(int argc, char **argv)
{
	if(argc < 3){ fprintf(stderr, "usage: insert_sanitize <golden dir> <scratch dir>\n"); return 2; }
	if(plan_checks() || retire_checks() || bloom_checks(argv[1], argv[2])){ return 1; }
	printf("live insert planning under sanitizers: %ld checks, %ld refusals, no report\n", checks, refused);
	return 0;
}
