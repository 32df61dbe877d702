// tests/sanitize/union_walk_driver.cpp -- the union steps of the walks of tests/union_walk.py through the library's own
// host-side planning (kwage_amd/csrc/union_plan.hpp: union_refusal, plan_union, union_unit_value; copy_plan.hpp
// copy_keep_mask) under -fsanitize=address,undefined: what tests/test_union_walk.py compares the model with.  No device.
// A step brings its own state as text: the destination's layout, the source's valid mask and rows, the lists, and the
// destination's rows in the units the caller expects to be written.  The program makes every (row, unit) as a lane of
// union_columns_kernel makes it -- the unit's value from loads of the source rows, OR what copy_keep_mask keeps of the
// destination's bytes, for the owners of a row's first and last unit -- and prints what the call returns and the rows
// written.
//   union_walk_driver < steps
// A step (tokens separated by white space; <hex> is "-" for no bytes):
//   union <same 0|1> <L dst> <L src> <dst next_byte> <dst tail_open> <dst tail_column> <dst stride> <src span> <src stride>
//         <rows sent> <src bytes per row sent> <first dst unit sent> <dst units sent> <n_sets> <members>
//   <hex of the source's valid mask> <n_sets + 1 offsets> <members columns>
//   <rows sent> x <hex of a source row>   <rows sent> x <hex of the destination row's units sent>
// Output per step:
//   union rc=0 first=.. sets=.. members=.. entries=.. first_unit=.. units=.. bytes_written=..   and per row: w <hex of the units written>
//   union rc=<code> error=<kwage_last_error()>                                               for a refused step
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "union_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static bool unhex(const std::string &s, std::vector<uint8_t> &out, size_t want)
{
	out.clear();
	if(s != "-"){
		if(s.size() % 2){ return false; }
		for(size_t i = 0; i < s.size(); i += 2){
			unsigned v = 0;
			if(sscanf(s.c_str() + i, "%2x", &v) != 1){ return false; }
			out.push_back((uint8_t)v);
		}
	}
	return out.size() == want;
}

int main()
{
	const int context = 0;
	std::string word;
	long ops = 0;
	while(std::cin >> word){
		if(word != "union"){ fprintf(stderr, "FAILED: unknown step %s\n", word.c_str()); return 1; }
		++ops;
		uint64_t same = 0, Ld = 0, Ls = 0, next_byte = 0, tail_open = 0, tail_column = 0, dst_stride = 0, src_span = 0, src_stride = 0;
		uint64_t nrows = 0, src_bytes = 0, unit0 = 0, units_sent = 0, n_sets = 0, members = 0;
		std::cin >> same >> Ld >> Ls >> next_byte >> tail_open >> tail_column >> dst_stride >> src_span >> src_stride
		         >> nrows >> src_bytes >> unit0 >> units_sent >> n_sets >> members;
		std::string hex;
		std::cin >> hex;
		std::vector<uint8_t> valid;
		if(!std::cin || !unhex(hex, valid, (size_t)((src_span + 7)/8))){ fprintf(stderr, "FAILED: step %ld: the valid mask\n", ops); return 1; }
		// (exactly as long as the span says: a look at a column at or beyond the span is a sanitizer report)
		std::vector<uint64_t> offsets(n_sets + 1), columns(members);
		for(auto &o : offsets){ std::cin >> o; }
		for(auto &c : columns){ std::cin >> c; }
		std::vector<std::vector<uint8_t>> src(nrows), dst(nrows);
		for(auto &r : src){ std::cin >> hex; if(!unhex(hex, r, (size_t)src_bytes)){ fprintf(stderr, "FAILED: step %ld: a source row\n", ops); return 1; } }
		for(auto &r : dst){ std::cin >> hex; if(!unhex(hex, r, (size_t)(16*units_sent))){ fprintf(stderr, "FAILED: step %ld: a destination row\n", ops); return 1; } }
		if(!std::cin){ fprintf(stderr, "FAILED: step %ld is cut short\n", ops); return 1; }

		const CopySide d = {&context, false, {15, 2, (uint32_t)Ld, 0}}, s = {&context, false, {15, 2, (uint32_t)Ls, 0}};
		// (a list of no members is a non-NULL pointer to nothing, as Group.union_columns passes it)
		const uint64_t none = 0;
		int rc = union_refusal(&d, &s, true, offsets.data(), true, (uint32_t)n_sets, false);
		UnionPlan plan;
		if(!rc){
			rc = plan_union(columns.empty() ? &none : columns.data(), offsets.data(), (uint32_t)n_sets, src_span, valid.data(), same != 0,
			                next_byte, tail_open != 0, tail_column, dst_stride, plan);
		}
		if(rc){
			printf("union rc=%d error=%s\n", rc, kwage_last_error());
			continue;
		}
		if(plan.first_unit < unit0 || plan.first_unit + plan.units > unit0 + units_sent || (plan.first_unit + plan.units)*16 > dst_stride){
			fprintf(stderr, "FAILED: step %ld: units [%llu, %llu) are written, [%llu, %llu) were expected\n", ops, (unsigned long long)plan.first_unit,
			        (unsigned long long)(plan.first_unit + plan.units), (unsigned long long)unit0, (unsigned long long)(unit0 + units_sent));
			return 1;
		}
		printf("union rc=0 first=%llu sets=%llu members=%llu entries=%llu first_unit=%llu units=%llu bytes_written=%llu\n", (unsigned long long)plan.first,
		       (unsigned long long)plan.n, (unsigned long long)plan.members, (unsigned long long)plan.entries.size(), (unsigned long long)plan.first_unit,
		       (unsigned long long)plan.units, (unsigned long long)((1ull << Ld)*plan.units*16));
		bool in_bounds = true, read_what_is_written = false;
		auto entry = [&](uint64_t i) {
			if(i >= plan.entries.size()){ in_bounds = false; return UnionEntry{0, 0, 0, 0}; }
			return plan.entries[i];
		};
		auto load = [&](uint64_t byte) {
			const uint64_t row = byte/src_stride, at = byte % src_stride;
			if(byte % 4 != 0 || row >= nrows || at + 4 > src_bytes){ in_bounds = false; return 0u; }
			if(same && at >= 16*plan.first_unit){ read_what_is_written = true; }
			uint32_t v;
			memcpy(&v, src[row].data() + at, 4);
			return v;
		};
		const uint64_t last_unit = plan.first_unit + plan.units - 1;
		const bool keeps_low = plan.first % 128 != 0, keeps_high = ((plan.first + plan.n - 1)/32) % 4 != 3;      // (union_columns_kernel's)
		for(uint64_t row = 0; row < nrows; ++row){
			printf("w ");
			for(uint64_t unit = plan.first_unit; unit <= last_unit; ++unit){
				uint32_t w[4], keep[4], old[4];
				union_unit_value(entry, load, plan.offsets.data(), row, src_stride, plan.first, plan.n, unit, w);
				copy_keep_mask(plan.first, plan.n, unit, keep);
				memcpy(old, dst[row].data() + 16*(unit - unit0), 16);
				if((keeps_low && unit == plan.first_unit) || (keeps_high && unit == last_unit)){
					for(int j = 0; j < 4; ++j){ w[j] |= old[j] & keep[j]; }
				}
				else if(keep[0] | keep[1] | keep[2] | keep[3]){ fprintf(stderr, "FAILED: step %ld: unit %llu keeps bytes nobody reads\n", ops, (unsigned long long)unit); return 1; }
				uint8_t out[16];
				memcpy(out, w, 16);
				for(int j = 0; j < 16; ++j){ printf("%02x", out[j]); }
			}
			printf("\n");
		}
		if(!in_bounds || read_what_is_written){
			fprintf(stderr, "FAILED: step %ld: %s\n", ops, !in_bounds ? "a load or an entry outside the source rows' bytes or the table" : "a load of a unit that is written");
			return 1;
		}
	}
	printf("%ld operations, no report\n", ops);
	return 0;
}
