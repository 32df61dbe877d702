// tests/sanitize/family_model_driver.cpp -- group_model_driver.cpp for SEVERAL named groups: the library's host-side planners
// (kwage_amd/csrc/insert_plan.hpp, compact_plan.hpp, fold_plan.hpp, copy_plan.hpp) driven by a stream of operations, under
// -fsanitize=address,undefined: what tests/test_family_model.py compares the family of tests/family_model.py with.  No
// device.  The program keeps what a group keeps on the host -- the valid mask, next_byte, the tail, finalized, the column
// count -- exactly as insert.hip's commit_insert, compact.hip, fold.hip and loader.hip's group_reserve_columns update them,
// and prints after every operation what the call returns and the state of the group it made or changed.
//   family_model_driver < operations
// Operations, one per line (a group is named by a word):
//   new <g> <L> <stride bytes> | close <g> | add <g> <num_filter> | ins <g> <n> | ret <g> <n> <columns ...>
//   set <g> <n> <columns ...> | cmp <g> | fin <g> | fold <src> <L2> <new g> | copy <dst> <src> <n, -1: all> <columns ...>
// Output, one line per operation:
//   <op> rc=<code> [...] | L=.. span=.. open=.. tail=.. columns=.. final=.. valid=<hex of the mask up to the span>
//   fold rc=.. units=.. read=.. written=..          and the state of the NEW group (refused: of the source)
//   copy rc=.. first=.. runs=.. first_unit=.. units=..   and the state of the destination
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "compact_plan.hpp"
#include "copy_plan.hpp"
#include "fold_plan.hpp"
#include "insert_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

struct Group {
	uint32_t L = 0;
	uint64_t stride = 0, next_byte = 0, tail_column = 0, num_columns = 0;
	bool tail_open = false, finalized = false;
	std::vector<uint8_t> h_valid;
};

static void print_state(const Group &g)
{
	printf(" | L=%u span=%llu open=%d tail=%llu columns=%llu final=%d valid=", g.L, (unsigned long long)(8*g.next_byte), (int)g.tail_open,
	       (unsigned long long)g.tail_column, (unsigned long long)g.num_columns, (int)g.finalized);
	for(uint64_t b = 0; b < g.next_byte; ++b){ printf("%02x", g.h_valid[b]); }
	// nothing valid may lie at or above the span
	for(uint64_t b = g.next_byte; b < g.stride; ++b){ if(g.h_valid[b]){ printf(" STRAY"); break; } }
	printf("\n");
}

// insert.hip commit_insert: the columns become valid, the tail opens behind them
static void commit_insert(Group &g, uint64_t first, uint64_t n)
{
	for(uint64_t c = first; c < first + n; ++c){ g.h_valid[c/8] |= (uint8_t)(1u << (c%8)); }
	g.tail_column = first + n;
	g.tail_open = true;
	g.next_byte = (first + n + 7)/8;
	g.num_columns += n;
}

int main()
{
	std::map<std::string, Group> groups;
	const int context = 0;                     // (every group lives on one context)
	std::string line;
	long ops = 0;
	while(std::getline(std::cin, line)){
		std::istringstream in(line);
		std::string op, name;
		if(!(in >> op >> name)){ continue; }
		++ops;
		if(op == "new"){
			Group g;
			in >> g.L >> g.stride;
			g.h_valid.assign(g.stride, 0);
			if(groups.count(name)){ fprintf(stderr, "FAILED: %s exists\n", name.c_str()); return 1; }
			groups[name] = g;
			printf("new rc=0");
			print_state(groups[name]);
			continue;
		}
		if(op == "fold"){
			// fold.hip kwage_group_fold: name is the SOURCE
			uint32_t L2 = 0;
			std::string made;
			in >> L2 >> made;
			if(!groups.count(name) || groups.count(made)){ fprintf(stderr, "FAILED: fold %s -> %s\n", name.c_str(), made.c_str()); return 1; }
			const Group &src = groups[name];
			const int rc = fold_refusal(true, true, false, src.L, L2, false);
			if(rc){
				printf("fold rc=%d units=0 read=0 written=0", rc);
				print_state(src);
				continue;
			}
			const FoldPlan plan = plan_fold(src.L, L2, src.next_byte, src.stride, 256);
			Group g;                               // kwage_group_create: the same stride, nothing in it
			g.L = L2;
			g.stride = src.stride;
			// the column layout is the source's, number for number
			g.next_byte = src.next_byte;
			g.tail_column = src.tail_column;
			g.tail_open = src.tail_open;
			g.num_columns = src.num_columns;
			g.h_valid = src.h_valid;
			g.finalized = src.finalized;
			groups[made] = g;
			printf("fold rc=0 units=%llu read=%llu written=%llu", (unsigned long long)plan.units_per_row, (unsigned long long)plan.bytes_read,
			       (unsigned long long)plan.bytes_written);
			print_state(groups[made]);
			continue;
		}
		if(!groups.count(name)){ fprintf(stderr, "FAILED: no group %s\n", name.c_str()); return 1; }
		if(op == "close"){
			groups.erase(name);
			printf("close rc=0\n");
			continue;
		}
		Group &g = groups[name];
		if(op == "copy"){
			// copy.hip kwage_group_copy_columns: name is the DESTINATION
			std::string from;
			long long n = 0;
			in >> from >> n;
			if(!groups.count(from)){ fprintf(stderr, "FAILED: no group %s\n", from.c_str()); return 1; }
			const Group &src = groups[from];
			std::vector<uint64_t> cols((size_t)std::max<long long>(n, 0));
			for(auto &c : cols){ in >> c; }
			const bool have_columns = n >= 0;
			const uint64_t count = have_columns ? (uint64_t)n : 0;
			const CopySide d = {&context, false, {15, 2, g.L, 0}}, s = {&context, false, {15, 2, src.L, 0}};
			int rc = copy_refusal(&d, &s, &g == &src, true, have_columns, count, false);
			CopyPlan plan;
			// (a list of no columns is a non-NULL pointer with n == 0: refused above, never planned)
			if(!rc){ rc = plan_copy(have_columns ? cols.data() : nullptr, count, src.next_byte*8, src.h_valid.data(), g.next_byte, g.tail_open, g.tail_column, g.stride, plan); }
			if(rc){ printf("copy rc=%d first=0 runs=0 first_unit=0 units=0", rc); }
			else{
				uint64_t first = 0;
				if(plan_insert(g.next_byte, g.tail_open, g.tail_column, g.stride, plan.n, &first) || first != plan.first){
					fprintf(stderr, "FAILED: plan_copy and plan_insert disagree\n");
					return 1;
				}
				commit_insert(g, plan.first, plan.n);
				printf("copy rc=0 first=%llu runs=%llu first_unit=%llu units=%llu", (unsigned long long)plan.first, (unsigned long long)plan.runs.size(),
				       (unsigned long long)plan.first_unit, (unsigned long long)plan.units);
			}
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
				commit_insert(g, first, n);
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
			const int rc = plan_compact(g.h_valid.data(), span, g.tail_open, g.tail_column, true, span, plan);
			if(rc){ printf("cmp rc=%d", rc); }
			else{
				compact_valid_mask(g.h_valid.data(), old_bytes, plan.m);
				g.next_byte = (plan.m + 7)/8;
				g.tail_column = plan.m;
				g.tail_open = true;
				printf("cmp rc=0 before=%llu after=%llu m=%llu runs=%llu nothing=%d units=%llu", (unsigned long long)span,
				       (unsigned long long)(8*g.next_byte), (unsigned long long)plan.m, (unsigned long long)plan.runs.size(),
				       (int)plan.nothing_to_close, (unsigned long long)(plan.end_unit - plan.first_unit));
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
