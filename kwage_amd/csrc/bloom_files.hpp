// kwage_amd/csrc/bloom_files.hpp -- `.bloom` files as the inputs of the database builder (builder.hip, kwage_build_db) and of
// the live insert (insert.hip, kwage_group_insert_bloom_files): opened, mapped and validated the way build_db() validates
// them (build_db.cpp:48-181, CRC32 :343-362) before anything is written.  Host code only: no device is touched.
//
// `.bloom` file = binary_write<BloomFilter> (binary_io.cpp:182-208): 1 magic byte (0xFF complete),
// BloomParam {u32 kmer_len, u32 log_2_filter_len, u32 num_hash, i32 hash_func} (bloom.h:546-556),
// u32 crc32 of the bit array, FilterInfo (binary_io.cpp:154-163), then 2^L/8 bytes of bits.
#ifndef KWAGE_AMD_BLOOM_FILES_HPP
#define KWAGE_AMD_BLOOM_FILES_HPP

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "host.hpp"
#include "internal.h"

namespace kwage {

struct BloomFile {
	int fd = -1;
	const unsigned char *map = nullptr;
	size_t size = 0;
	uint32_t crc = 0;
	FilterInfo info;
	size_t bits_off = 0;
	void close_file()
	{
		if(map){ munmap((void*)map, size); map = nullptr; }
		if(fd >= 0){ close(fd); fd = -1; }
	}
};

// f(0) ... f(nparts - 1), on threads of their own where they can be had.  A thread that cannot be created
// (std::system_error -- which must never cross the C ABI) leaves its part to the caller.
template <typename F>
void run_parts(unsigned nparts, F f)
{
	std::vector<std::thread> pool;
	std::vector<unsigned> mine;
	for(unsigned t = 1; t < nparts; ++t){
		try{ pool.emplace_back(f, t); }
		catch(...){ mine.push_back(t); }
	}
	if(nparts){ f(0u); }
	for(unsigned t : mine){ f(t); }
	for(auto &th : pool){ th.join(); }
}

inline uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// Opens and maps the n files into `files` (resized to n) and checks every one: complete, the parameters `params`, a
// readable FilterInfo, 2^L/8 bytes of bits whose CRC32 (host threads) is the one the file states.  Messages start with
// `who`.  On any error every file is closed again and the status returned: KWAGE_ERR_IO (cannot be opened or mapped),
// KWAGE_ERR_FORMAT (truncated, incomplete, bad record, bad CRC32) or KWAGE_ERR_ARG (other parameters).
inline int open_bloom_files(const char *who, const char *const *bloom_paths, uint32_t n, const kwage_params *params, std::vector<BloomFile> &files)
{
	const uint64_t filter_bytes = ((1ull << params->log_2_filter_len) + 7)/8;
	files.clear();
	files.resize(n);
	auto cleanup = [&]() { for(auto &f : files){ f.close_file(); } };

	// ---- open + validate every .bloom file (build_db.cpp:48-181) ------------------------------
	for(uint32_t i = 0; i < n; ++i){
		BloomFile &f = files[i];
		if(!bloom_paths[i]){ cleanup(); return fail(KWAGE_ERR_ARG, "%s: NULL Bloom filter file name", who); }
		f.fd = open(bloom_paths[i], O_RDONLY);
		struct stat st;
		if(f.fd < 0 || fstat(f.fd, &st) != 0){ cleanup(); return fail(KWAGE_ERR_IO, "%s: Unable to open Bloom filter file %s", who, bloom_paths[i]); }
		f.size = (size_t)st.st_size;
		if(f.size < 21){ cleanup(); return fail(KWAGE_ERR_FORMAT, "%s: %s is truncated", who, bloom_paths[i]); }
		f.map = (const unsigned char*)mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0);
		if(f.map == MAP_FAILED){ f.map = nullptr; cleanup(); return fail(KWAGE_ERR_IO, "%s: mmap(%s) failed", who, bloom_paths[i]); }
		if(f.map[0] != 0xFF){ cleanup(); return fail(KWAGE_ERR_FORMAT, "%s: Incomplete Bloom filter %s", who, bloom_paths[i]); }
		const uint32_t k = rd32(f.map + 1), lg = rd32(f.map + 5), nh = rd32(f.map + 9);
		const int32_t hf = (int32_t)rd32(f.map + 13);
		if(k != params->kmer_len || lg != params->log_2_filter_len || nh != params->num_hash || hf != params->hash_func){
			cleanup();
			return fail(KWAGE_ERR_ARG, "%s: Inconsistent Bloom parameters in %s", who, bloom_paths[i]);
		}
		f.crc = rd32(f.map + 17);
		size_t used = 0;
		if(!parse_filter_info(f.map + 21, f.size - 21, f.info, &used)){ cleanup(); return fail(KWAGE_ERR_FORMAT, "%s: Error reading Bloom filter info from %s", who, bloom_paths[i]); }
		f.bits_off = 21 + used;
		if(f.size - f.bits_off < filter_bytes){ cleanup(); return fail(KWAGE_ERR_FORMAT, "%s: Error reading filter bytes from %s", who, bloom_paths[i]); }
	}

	// ---- per-filter CRC32 (build_db.cpp:343-362), host threads; checked BEFORE anything is written
	{
		const unsigned nthread = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
		std::atomic<uint32_t> next(0), bad(0xFFFFFFFFu);
		run_parts(nthread, [&](unsigned) {
			for(uint32_t i = next++; i < n; i = next++){
				uint64_t crc = crc32_z(0L, Z_NULL, 0);
				crc = crc32_z(crc, files[i].map + files[i].bits_off, filter_bytes);
				if((uint32_t)crc != files[i].crc){ bad = i; }
			}
		});
		if(bad != 0xFFFFFFFFu){
			const uint32_t i = bad;
			cleanup();
			return fail(KWAGE_ERR_FORMAT, "%s: One or more invalid Bloom filter CRC32 values (%s)", who, bloom_paths[i]);
		}
	}
	return KWAGE_OK;
}

}  // namespace kwage

#endif
