// tests/sanitize/build_plan_sanitize.cpp -- the host-side planning of the builder and the re-pack
// (kwage_amd/csrc/build_plan.hpp: rows per chunk, chunks, the stride of the filters in the device's input block) under
// -fsanitize=address,undefined.  No device: the functions take plain values.  Reads a file of cases, one per line,
//   <id> B <budget_bytes> <n> <filter_len> <pad_bytes or -1>
//   <id> R <budget_bytes> <nrows> <dst_words> <max_width>
// and prints each plan (tests/test_build_plan.py holds the expectations and the invariants).
//   build_plan_sanitize cases.txt
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "build_plan.hpp"

using namespace kwage;

int main(int argc, char **argv)
{
	if(argc != 2){ fprintf(stderr, "usage: build_plan_sanitize cases.txt\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if(!f){ fprintf(stderr, "FAILED: cannot open %s\n", argv[1]); return 2; }
	long cases = 0;
	for(;;){
		long id;
		char kind;
		uint64_t budget, a, b;
		long long c;
		const int got = fscanf(f, "%ld %c %" SCNu64 " %" SCNu64 " %" SCNu64 " %lld", &id, &kind, &budget, &a, &b, &c);
		if(got == EOF){ break; }
		if(got != 6 || (kind != 'B' && kind != 'R') || (kind == 'R' && c < 0)){ fprintf(stderr, "FAILED: bad case line %ld\n", cases); fclose(f); return 2; }
		if(kind == 'B'){
			const BuildChunks p = plan_build_chunks(budget, a, b, c);
			printf("case %ld chunk_rows=%" PRIu64 " in_stride=%" PRIu64 " chunks=%" PRIu64 "\n", id, p.chunk_rows, p.in_stride, p.chunks);
		}
		else{
			const RepackChunks p = plan_repack_chunks(budget, a, b, (uint64_t)c);
			printf("case %ld chunk_rows=%" PRIu64 " chunks=%" PRIu64 "\n", id, p.chunk_rows, p.chunks);
		}
		++cases;
	}
	fclose(f);
	printf("build planning under sanitizers: %ld cases, no report\n", cases);
	return 0;
}
