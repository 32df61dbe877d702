// tests/sanitize/group_model_driver.cpp -- the library's own host-side planners (kwage_amd/csrc/insert_plan.hpp,
// compact_plan.hpp) driven by a stream of operations, under -fsanitize=address,undefined: what tests/test_group_model.py
// compares the model of tests/group_model.py with.  No device.  The program keeps what a group keeps on the host -- the
// valid mask, next_byte, the tail, finalized, the column count -- exactly as insert.hip, compact.hip and loader.hip's
// group_reserve_columns update them, and prints after every operation what the call returns and the state it leaves.
//   group_model_driver < operations
// Operations, one per line:
//   new <stride bytes> | add <num_filter> | ins <n> | ret <n> <columns ...> | set <n> <columns ...> | cmp | fin
// Output, one line per operation:
//   <op> rc=<code> [first=.. word_first=.. word_last=.. keep=..] [distinct=..] [before=.. after=.. m=.. runs=.. nothing=.. units=.. map=src:dst:len,..]
//        | span=.. open=.. tail=.. columns=.. valid=<hex of the mask up to the span>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "compact_plan.hpp"
#include "insert_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

struct Group {
	uint64_t stride = 0, next_byte = 0, tail_column = 0, num_columns = 0;
	bool tail_open = false, finalized = false;
	std::vector<uint8_t> h_valid;
};

static void print_state(const Group &g)
{
	printf(" | span=%llu open=%d tail=%llu columns=%llu valid=", (unsigned long long)(8*g.next_byte), (int)g.tail_open,
	       (unsigned long long)g.tail_column, (unsigned long long)g.num_columns);
	for(uint64_t b = 0; b < g.next_byte; ++b){ printf("%02x", g.h_valid[b]); }
	// nothing valid may lie at or above the span
	for(uint64_t b = g.next_byte; b < g.stride; ++b){ if(g.h_valid[b]){ printf(" STRAY"); break; } }
	printf("\n");
}

int main()
{
	Group g;
	std::string line;
	long ops = 0;
	while(std::getline(std::cin, line)){
		std::istringstream in(line);
		std::string op;
		if(!(in >> op)){ continue; }
		++ops;
		if(op == "new"){
			g = Group();
			in >> g.stride;
			g.h_valid.assign(g.stride, 0);
			printf("new rc=0");
		}
		else if(op == "add"){
			// loader.hip group_reserve_columns
			uint64_t nf = 0;
			in >> nf;
			const uint64_t start = (g.next_byte + 15)/16*16, width = (nf + 7)/8;
			int rc = 0;
			if(g.finalized){ rc = KWAGE_ERR_STATE; }
			else if(nf == 0 || start + width > g.stride){ rc = KWAGE_ERR_ARG; }
			else{
				for(uint64_t c = 0; c < nf; ++c){ g.h_valid[start + c/8] |= (uint8_t)(1u << (c%8)); }
				g.next_byte = start + width;
				g.num_columns += nf;
				g.tail_open = false;
			}
			printf("add rc=%d first=%llu", rc, (unsigned long long)(rc ? 0 : 8*start));
		}
		else if(op == "ins"){
			// insert.hip insert_prepare + commit_insert
			uint64_t n = 0, first = 0;
			in >> n;
			const int rc = plan_insert(g.next_byte, g.tail_open, g.tail_column, g.stride, n, &first);
			if(rc){ printf("ins rc=%d first=0 word_first=0 word_last=0 keep=0", rc); }
			else{
				const InsertSpan sp = insert_span(first, n);
				for(uint64_t c = first; c < first + n; ++c){ g.h_valid[c/8] |= (uint8_t)(1u << (c%8)); }
				g.tail_column = first + n;
				g.tail_open = true;
				g.next_byte = (first + n + 7)/8;
				g.num_columns += n;
				printf("ins rc=0 first=%llu word_first=%llu word_last=%llu keep=%u", (unsigned long long)first,
				       (unsigned long long)sp.word_first, (unsigned long long)sp.word_last, sp.keep_bits);
			}
		}
		else if(op == "ret"){
			// insert.hip kwage_group_retire_columns
			uint64_t n = 0, distinct = 0;
			in >> n;
			std::vector<uint64_t> cols(n);
			for(auto &c : cols){ in >> c; }
			std::vector<RetirePair> pairs;
			const int rc = n ? plan_retire(g.h_valid.data(), g.next_byte*8, cols.data(), n, pairs, &distinct) : 0;
			if(!rc){
				for(const RetirePair &p : pairs){
					for(uint32_t k = 0; k < 4; ++k){ g.h_valid[4*p.word + k] &= (uint8_t)~(p.mask >> (8*k)); }
				}
				g.num_columns -= distinct;
			}
			printf("ret rc=%d distinct=%llu", rc, (unsigned long long)(rc ? 0 : distinct));
		}
		else if(op == "set"){
			// loader.hip kwage_group_set_bits: the columns' bound
			uint64_t n = 0;
			in >> n;
			int rc = 0;
			for(uint64_t i = 0; i < n; ++i){
				uint64_t c = 0;
				in >> c;
				if(c >= g.next_byte*8){ rc = KWAGE_ERR_ARG; }
			}
			printf("set rc=%d", rc);
		}
		else if(op == "cmp"){
			// compact.hip kwage_group_compact
			const uint64_t old_bytes = g.next_byte, span = old_bytes*8;
			CompactPlan plan;
			std::vector<uint64_t> map(span ? span : 1);
			const int rc = plan_compact(g.h_valid.data(), span, g.tail_open, g.tail_column, true, span, plan);
			if(rc){ printf("cmp rc=%d", rc); }
			else{
				compact_fill_map(g.h_valid.data(), span, map.data());
				compact_valid_mask(g.h_valid.data(), old_bytes, plan.m);
				g.next_byte = (plan.m + 7)/8;
				g.tail_column = plan.m;
				g.tail_open = true;
				printf("cmp rc=0 before=%llu after=%llu m=%llu runs=%llu nothing=%d units=%llu map=", (unsigned long long)span,
				       (unsigned long long)(8*g.next_byte), (unsigned long long)plan.m, (unsigned long long)plan.runs.size(),
				       (int)plan.nothing_to_close, (unsigned long long)(plan.end_unit - plan.first_unit));
				// the map, folded: stretches of columns whose new numbers count up with them
				uint64_t c = 0;
				bool any = false;
				while(c < span){
					if(map[c] == 0xFFFFFFFFFFFFFFFFull){ ++c; continue; }
					uint64_t len = 1;
					while(c + len < span && map[c + len] == map[c] + len){ ++len; }
					printf("%s%llu:%llu:%llu", any ? "," : "", (unsigned long long)c, (unsigned long long)map[c], (unsigned long long)len);
					any = true;
					c += len;
				}
				if(!any){ printf("-"); }
			}
		}
		else if(op == "fin"){
			g.finalized = true;
			printf("fin rc=0");
		}
		else{
			fprintf(stderr, "FAILED: unknown operation %s\n", op.c_str());
			return 1;
		}
		print_state(g);
	}
	printf("%ld operations, no report\n", ops);
	return 0;
}
