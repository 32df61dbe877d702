// kwage_amd/csrc/compact_plan.hpp -- the host-side planning of the compaction (compact.hip, kwage_group_compact): the runs
// the surviving columns fold into, the part of a row that is rewritten, the schedule of a row as data, and -- written ONCE
// for the kernel and the host -- how one 16-byte destination unit is made from loads.  The address arithmetic is
// save_plan.hpp's; nothing of it is restated here.  Plain functions of plain values: no device, no group --
// tests/sanitize/compact_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_COMPACT_PLAN_HPP
#define KWAGE_AMD_COMPACT_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "save_plan.hpp"

namespace kwage {

// What a compaction does to a group whose valid mask is valid[] (a bit per column, LSB first) over `span` columns, the
// open tail (if any) at `tail`:
//   runs                   destination columns 0 .. m - 1 = the valid columns in ascending order, folded by plan_save's rule
//                          (a column that follows its predecessor's source extends the run); src_first >= dst_first in every run
//   first_unit, end_unit   the 16-byte units of a row that are rewritten: with p the first invalid column, every unit wholly
//                          below p keeps its bytes; units up to the end of the old span are written, zero at and above bit m
//   nothing_to_close       every column below the tail is valid: no unit is rewritten (first_unit == end_unit)
struct CompactPlan {
	uint64_t span_before = 0, m = 0, first_unit = 0, end_unit = 0;
	bool nothing_to_close = true;
	std::vector<SaveRun> runs;
};

inline bool compact_is_valid(const uint8_t *valid, uint64_t c) { return (valid[c/8] >> (c%8)) & 1; }

// Refused (KWAGE_ERR_ARG, the plan untouched but for its cleared runs): a column map of fewer than `span` entries
// (capacity counts only where want_map), more valid columns than a run's 32-bit destination holds.
inline int plan_compact(const uint8_t *valid, uint64_t span, bool tail_open, uint64_t tail, bool want_map, uint64_t capacity, CompactPlan &plan)
{
	const char *who = "kwage_group_compact";
	plan.runs.clear();
	if(want_map && capacity < span){
		return fail(KWAGE_ERR_ARG, "%s: new_column holds %llu entries, the span is %llu", who, (unsigned long long)capacity, (unsigned long long)span);
	}
	uint64_t m = 0, p = span;
	for(uint64_t c = 0; c < span; ++c){
		if(compact_is_valid(valid, c)){ ++m; }
		else if(p == span){ p = c; }
	}
	if(m > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: %llu columns do not fit a run table", who, (unsigned long long)m); }
	uint64_t d = 0;
	for(uint64_t c = 0; c < span; ++c){
		if(!compact_is_valid(valid, c)){ continue; }
		if(!plan.runs.empty() && c == plan.runs.back().src_first + plan.runs.back().len){ ++plan.runs.back().len; }
		else{ plan.runs.push_back(SaveRun{c, (uint32_t)d, 1u}); }
		++d;
	}
	plan.span_before = span;
	plan.m = m;
	plan.nothing_to_close = p >= (tail_open ? std::min(tail, span) : span);
	plan.first_unit = plan.nothing_to_close || m == 0 ? 0 : p/128;
	plan.end_unit = plan.nothing_to_close || m == 0 ? plan.first_unit : (span + 127)/128;
	return KWAGE_OK;
}

// new_column[c] for every c < span: the number of valid columns below c, or KWAGE_NO_COLUMN for a pad or retired column.
inline void compact_fill_map(const uint8_t *valid, uint64_t span, uint64_t *new_column)
{
	uint64_t d = 0;
	for(uint64_t c = 0; c < span; ++c){ new_column[c] = compact_is_valid(valid, c) ? d++ : 0xFFFFFFFFFFFFFFFFull; }
}

// The valid mask afterwards: exactly bits [0, m), everything up to old_bytes cleared.
inline void compact_valid_mask(uint8_t *valid, uint64_t old_bytes, uint64_t m)
{
	std::fill(valid, valid + old_bytes, (uint8_t)0);
	for(uint64_t c = 0; c < m/8; ++c){ valid[c] = 0xFF; }
	if(m % 8){ valid[m/8] = (uint8_t)((1u << (m%8)) - 1u); }
}

// The schedule of a row, as data.  The units [first_unit, end_unit) of a row are taken in segments of S = `lanes`
// consecutive units, left to right; `lanes` threads share a row (a power of two, 8 .. threads) and threads / lanes rows share
// a workgroup.  In segment `seg` thread `lane` of its row makes unit first_unit + seg*lanes + lane.  ALL units of a segment
// are made before ANY of them is stored (compact_kernels.hpp: a workgroup barrier between the two).
struct CompactSchedule {
	uint32_t lanes, rows_per_wg;
	uint64_t segments;
};
inline CompactSchedule compact_schedule(uint64_t first_unit, uint64_t end_unit, uint32_t threads)
{
	CompactSchedule s;
	const uint64_t units = end_unit - first_unit;
	s.lanes = 8;
	while(s.lanes < threads && s.lanes < units){ s.lanes *= 2; }
	s.rows_per_wg = threads/s.lanes;
	s.segments = (units + s.lanes - 1)/s.lanes;
	return s;
}
KWAGE_HD inline uint64_t compact_unit_of(uint64_t first_unit, uint64_t seg, uint32_t lanes, uint32_t lane)
{
	return first_unit + seg*lanes + lane;
}

// Destination unit u (columns 128u .. 128u + 127) of row `row`, from loads: w[0..3] are its four words, zero at and above
// column m.  A unit inside ONE run takes save_unit_in_run's path, its loads requested together; any other unit -- one a run
// ends or begins in, the row's last one -- is walked piece by piece (save_word), the dword loaded last kept for the next
// piece; a unit at or above m is zero and loads nothing.  Every dword asked for lies at or above byte 16u of the row,
// because no run's source lies below its destination: the property the in-place schedule rests on.
// load(byte offset) returns the dword there, load4(byte offset) the 16 bytes at a 16-byte boundary.
template <typename LOAD, typename LOAD4>
KWAGE_HD inline void compact_unit(LOAD &&load, LOAD4 &&load4, const SaveRun *runs, uint32_t n_runs, uint32_t m,
                                  uint64_t row, uint64_t stride, uint64_t matrix_bytes, uint64_t u, uint32_t (&w)[4])
{
	const uint64_t d0 = 128*u;
	if(d0 >= m){
		w[0] = w[1] = w[2] = w[3] = 0u;
		return;
	}
	uint32_t k = save_find_run(runs, n_runs, (uint32_t)d0);
	const SaveRun first = runs[k];
	if(d0 + 128 <= (uint64_t)first.dst_first + first.len){
		save_unit_in_run(load, load4, row, stride, first.src_first + ((uint32_t)d0 - first.dst_first), w);
		return;
	}
	uint64_t have_byte = ~0ull;
	uint32_t have = 0;
	auto load_kept = [&](uint64_t byte) {
		if(byte != have_byte){
			have = load(byte);
			have_byte = byte;
		}
		return have;
	};
	for(int j = 0; j < 4; ++j){
		const uint64_t b = d0 + 32u*j;
		w[j] = b < m ? save_word(load_kept, runs, &k, row, stride, matrix_bytes, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + 32, m)) : 0u;
	}
}

}  // namespace kwage

#endif
