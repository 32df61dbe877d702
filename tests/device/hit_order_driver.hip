// tests/device/hit_order_driver.hip -- order_hits_by_runs (kwage_amd/csrc/hit_sort.hip) on tables and lists read from
// files, without a search in front of it: tests/test_gpu_hit_order.py writes the cases of tests/hit_order_cases.py,
// runs this program once over them and compares what it wrote with the numpy reference byte for byte.
//
//   hit_order_driver CASE...       for every CASE a file CASE.out is written
//
// CASE (little-endian):  uint64 n_runs, uint64 n_hits, uint64 table[n_runs] (first << 16 | records), kwage_hit raw[n_hits]
// CASE.out:              uint64 total (the word at *d_total), uint64 guards (bit 0: the band below the scratch block
//                        still holds the sentinel, bit 1: the band above it), kwage_hit ordered[n_hits] (from *d_ordered)
//
// The scratch block is exactly hit_order_scratch_bytes(n_hits, n_runs) long, lies between two guard bands and is filled,
// like them, with SENTINEL bytes before the call: records the table does not account for stay SENTINEL in the output.
// Every HIP call is checked; the first error ends the process with status 1 before another case is started.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "internal.h"

// the three device entry points host.cpp's kwage_make_bloom calls: not part of this build, and never called
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

namespace {

constexpr uint64_t GUARD_BYTES = 8192;
constexpr int SENTINEL = 0xA5;

#define HIP_OK(call)                                                                                         \
	do {                                                                                                     \
		const hipError_t e_ = (call);                                                                        \
		if(e_ != hipSuccess){                                                                                \
			fprintf(stderr, "hit_order_driver: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
			exit(1);                                                                                         \
		}                                                                                                    \
	} while(0)

[[noreturn]] void die(const std::string &what)
{
	fprintf(stderr, "hit_order_driver: %s\n", what.c_str());
	exit(1);
}

void read_all(FILE *f, void *to, uint64_t bytes, const std::string &path)
{
	if(bytes && fread(to, 1, bytes, f) != bytes){ die(path + ": file too short"); }
}

bool all_sentinel(const std::vector<unsigned char> &v)
{
	for(unsigned char c : v){ if(c != SENTINEL){ return false; } }
	return true;
}

void run_case(hipStream_t stream, const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if(!f){ die(path + ": cannot open"); }
	uint64_t head[2];
	read_all(f, head, sizeof(head), path);
	const uint64_t n_runs = head[0], n_hits = head[1];
	if(n_runs == 0 || n_hits == 0 || n_runs > (1ull << 28) || n_hits > (1ull << 28)){ die(path + ": n_runs / n_hits out of range"); }
	std::vector<uint64_t> table(n_runs);
	std::vector<kwage_hit> raw(n_hits);
	read_all(f, table.data(), n_runs*sizeof(uint64_t), path);
	read_all(f, raw.data(), n_hits*sizeof(kwage_hit), path);
	fclose(f);
	// (the call's own precondition, kept here too: a table that claims more than n_hits records could write outside the block)
	uint64_t claimed = 0;
	for(uint64_t e : table){
		const uint64_t n = e & 0xFFFF;
		if(n && (e >> 16) + n > n_hits){ die(path + ": a run lies outside the raw list"); }
		claimed += n;
	}
	if(claimed > n_hits){ die(path + ": the table claims more records than the list holds"); }

	const uint64_t scratch_bytes = kwage::hit_order_scratch_bytes(n_hits, n_runs);
	unsigned long long *d_table = nullptr;
	kwage_hit *d_raw = nullptr;
	unsigned char *d_block = nullptr;
	HIP_OK(hipMalloc((void**)&d_table, n_runs*sizeof(uint64_t)));
	HIP_OK(hipMalloc((void**)&d_raw, n_hits*sizeof(kwage_hit)));
	HIP_OK(hipMalloc((void**)&d_block, GUARD_BYTES + scratch_bytes + GUARD_BYTES));
	unsigned char *d_scratch = d_block + GUARD_BYTES;
	HIP_OK(hipMemcpyAsync(d_table, table.data(), n_runs*sizeof(uint64_t), hipMemcpyHostToDevice, stream));
	HIP_OK(hipMemcpyAsync(d_raw, raw.data(), n_hits*sizeof(kwage_hit), hipMemcpyHostToDevice, stream));
	HIP_OK(hipMemsetAsync(d_block, SENTINEL, GUARD_BYTES + scratch_bytes + GUARD_BYTES, stream));

	kwage_hit *d_ordered = nullptr;
	const uint64_t *d_total = nullptr;
	const int rc = kwage::order_hits_by_runs(stream, d_raw, n_hits, d_table, n_runs, d_scratch, scratch_bytes, &d_ordered, &d_total);
	if(rc != KWAGE_OK){ die(path + ": order_hits_by_runs: " + kwage_last_error()); }
	HIP_OK(hipStreamSynchronize(stream));
	HIP_OK(hipGetLastError());
	const unsigned char *lo = (const unsigned char*)d_ordered, *hi = lo + n_hits*sizeof(kwage_hit);
	const unsigned char *tw = (const unsigned char*)d_total;
	if(lo < d_scratch || hi > d_scratch + scratch_bytes || tw < d_scratch || tw + sizeof(uint64_t) > d_scratch + scratch_bytes){
		die(path + ": *d_ordered or *d_total lies outside the scratch block");
	}

	std::vector<kwage_hit> ordered(n_hits);
	std::vector<unsigned char> below(GUARD_BYTES), above(GUARD_BYTES);
	uint64_t total = 0;
	HIP_OK(hipMemcpy(ordered.data(), d_ordered, n_hits*sizeof(kwage_hit), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(&total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(below.data(), d_block, GUARD_BYTES, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(above.data(), d_scratch + scratch_bytes, GUARD_BYTES, hipMemcpyDeviceToHost));
	HIP_OK(hipFree(d_block));
	HIP_OK(hipFree(d_raw));
	HIP_OK(hipFree(d_table));

	const uint64_t out_head[2] = {total, (uint64_t)(all_sentinel(below) ? 1 : 0) | (uint64_t)(all_sentinel(above) ? 2 : 0)};
	const std::string out_path = path + ".out";
	FILE *o = fopen(out_path.c_str(), "wb");
	if(!o){ die(out_path + ": cannot create"); }
	if(fwrite(out_head, 1, sizeof(out_head), o) != sizeof(out_head) || fwrite(ordered.data(), sizeof(kwage_hit), n_hits, o) != n_hits || fclose(o) != 0){
		die(out_path + ": write failed");
	}
	printf("%s: n_runs %llu n_hits %llu scratch %llu total %llu guards %llu\n", path.c_str(), (unsigned long long)n_runs, (unsigned long long)n_hits,
	       (unsigned long long)scratch_bytes, (unsigned long long)total, (unsigned long long)out_head[1]);
	fflush(stdout);
}

}  // namespace

int main(int argc, char **argv)
{
	if(argc < 2){ die("usage: hit_order_driver CASE..."); }
	static_assert(sizeof(kwage_hit) == 12, "a hit record is three 32-bit words");
	HIP_OK(hipSetDevice(0));
	hipStream_t stream;
	HIP_OK(hipStreamCreate(&stream));
	for(int i = 1; i < argc; ++i){ run_case(stream, argv[i]); }
	HIP_OK(hipStreamDestroy(stream));
	return 0;
}
