// kwage_amd/csrc/copy_plan.hpp -- the host-side planning of the copy between groups (copy.hip, kwage_group_copy_columns):
// the refusals, the runs the column list folds into, where the columns go in the destination (the live insert's rule:
// insert_plan.hpp plan_insert), the 16-byte units of a destination row that are written, and -- written ONCE for the
// kernel and the host -- the value of one such unit.  The address arithmetic and the column checks are save_plan.hpp's;
// nothing of them is restated here.  Plain functions of plain values: no device, no group --
// tests/sanitize/copy_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_COPY_PLAN_HPP
#define KWAGE_AMD_COPY_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "insert_plan.hpp"
#include "save_plan.hpp"

namespace kwage {

// What a copy of `n` columns to destination columns first .. first + n - 1 does:
//   columns                the list the all-columns form stands for (the valid columns of the source, ascending); empty
//                          where the caller gave a list
//   runs                   SaveRun with dst_first RELATIVE to `first`: columns first + dst_first .. of the destination are
//                          columns src_first .. of the source
//   first_unit, units      the 16-byte units of a destination row that are stored: [first_unit, first_unit + units), from
//                          the unit that holds column `first` to the one that holds column first + n - 1
struct CopyPlan {
	uint64_t first = 0, n = 0, first_unit = 0, units = 0;
	std::vector<uint64_t> columns;
	std::vector<SaveRun> runs;
};

// What the refusals need to know of a group.
struct CopySide {
	const void *ctx;
	bool sparse;
	kwage_params params;
};

// The refusals of kwage_group_copy_columns that need no column list, in the order the call makes them; dst and src may be
// NULL.  (The pending search is KWAGE_ERR_STATE, everything else KWAGE_ERR_ARG.)
inline int copy_refusal(const CopySide *dst, const CopySide *src, bool same_group, bool have_first, bool have_columns, uint64_t n, bool search_pending)
{
	const char *who = "kwage_group_copy_columns";
	if(!dst || !src || !have_first){ return fail(KWAGE_ERR_ARG, "%s: NULL %s", who, !dst ? "dst" : !src ? "src" : "first_column"); }
	if(!have_columns && n != 0){ return fail(KWAGE_ERR_ARG, "%s: NULL columns with n = %llu", who, (unsigned long long)n); }
	if(have_columns && n == 0){ return fail(KWAGE_ERR_ARG, "%s: n is 0", who); }
	if(same_group){ return fail(KWAGE_ERR_ARG, "%s: dst and src are the same group", who); }
	if(dst->ctx != src->ctx){ return fail(KWAGE_ERR_ARG, "%s: the groups belong to different contexts", who); }
	if(dst->sparse || src->sparse){ return fail(KWAGE_ERR_ARG, "%s: a sparse group takes part in no copy", who); }
	const kwage_params &a = dst->params, &b = src->params;
	if(a.kmer_len != b.kmer_len){ return fail(KWAGE_ERR_ARG, "%s: kmer_len differs: dst %u, src %u", who, a.kmer_len, b.kmer_len); }
	if(a.num_hash != b.num_hash){ return fail(KWAGE_ERR_ARG, "%s: num_hash differs: dst %u, src %u", who, a.num_hash, b.num_hash); }
	if(a.log_2_filter_len != b.log_2_filter_len){ return fail(KWAGE_ERR_ARG, "%s: log_2_filter_len differs: dst %u, src %u", who, a.log_2_filter_len, b.log_2_filter_len); }
	if(a.hash_func != b.hash_func){ return fail(KWAGE_ERR_ARG, "%s: hash_func differs: dst %d, src %d", who, (int)a.hash_func, (int)b.hash_func); }
	if(search_pending){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); }
	return KWAGE_OK;
}

// The list (columns == NULL, n == 0: every valid column of the source, ascending) checked and folded, and placed in the
// destination.  Refused (KWAGE_ERR_ARG, the plan's runs empty), in this order: a source without valid columns in the
// all-columns form, n > 2^32 - 1, a column at or beyond the source's span, a pad or retired column of src_valid[] (a bit
// per column, LSB first), a column listed twice (save_plan.hpp save_check_columns), more columns than the destination's
// row holds behind where the next insert lands (plan_insert).
inline int plan_copy(const uint64_t *columns, uint64_t n, uint64_t src_span, const uint8_t *src_valid,
                     uint64_t dst_next_byte, bool dst_tail_open, uint64_t dst_tail_column, uint64_t dst_stride, CopyPlan &plan)
{
	const char *who = "kwage_group_copy_columns";
	plan.runs.clear();
	plan.columns.clear();
	if(!columns){
		for(uint64_t c = 0; c < src_span; ++c){ if((src_valid[c/8] >> (c%8)) & 1){ plan.columns.push_back(c); } }
		if(plan.columns.empty()){ return fail(KWAGE_ERR_ARG, "%s: src has no valid column", who); }
		columns = plan.columns.data();
		n = plan.columns.size();
	}
	if(n > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "%s: %llu columns do not fit a run table", who, (unsigned long long)n); }
	int rc = save_check_columns(who, columns, n, src_span, src_valid);
	if(rc){ return rc; }
	uint64_t first = 0;
	if((rc = plan_insert(dst_next_byte, dst_tail_open, dst_tail_column, dst_stride, n, &first))){ return rc; }
	save_fold_runs(columns, n, plan.runs);
	plan.first = first;
	plan.n = n;
	plan.first_unit = first/128;
	plan.units = (first + n + 127)/128 - plan.first_unit;
	return KWAGE_OK;
}

// What unit `unit` of a destination row keeps from memory, as a mask over its four words -- the call owns what the live
// insert owns, everything from first_column to the end of the last 32-bit WORD it touches (insert_plan.hpp insert_span):
// the bits below first_column in the first unit, and the words above the one that holds column first_column + n - 1 in
// the last unit.  (The latter are zero wherever no set bit lies at or above the group's span -- every state but the one a
// compaction of a group without valid columns leaves, which launches nothing and keeps what the memory held.)  All zero
// for every unit in between, for a first unit where first_column % 128 == 0 and a last unit whose last word is written.
KWAGE_HD inline void copy_keep_mask(uint64_t first_column, uint64_t n, uint64_t unit, uint32_t (&keep)[4])
{
	const uint64_t word_last = (first_column + n - 1)/32;
	for(int j = 0; j < 4; ++j){
		const uint64_t c0 = 128*unit + 32u*j;
		if(c0/32 > word_last){ keep[j] = 0xFFFFFFFFu; }
		else if(c0 >= first_column){ keep[j] = 0u; }
		else{ keep[j] = first_column - c0 >= 32 ? 0xFFFFFFFFu : ((1u << (first_column - c0)) - 1u); }
	}
}

// A whole 16-byte unit inside ONE run whose source columns start off a 16-byte boundary of the row: the four or five
// source dwords lie in TWO consecutive aligned 16-byte pieces, both requested together -- two loads per lane in place of
// save_unit_in_run's five, each covering 16 consecutive bytes of a wave's 1 KiB stretch of the row (a shift of one bit
// behind an open tail is this case for every unit of the copy; profiles/r12_copy_bench.txt, case b).  The second piece holds
// a dword the unit needs, which lies inside the matrix, and rows and the matrix end on 16-byte boundaries: the piece lies
// inside the matrix.  Which dwords are taken is said by masks, neither by an index nor by a branch: the words stay in registers,
// and the lanes of a wave whose runs start at different dwords do not part.
template <typename LOAD4>
KWAGE_HD inline void copy_unit_off_boundary(LOAD4 &&load4, uint64_t row, uint64_t stride, uint64_t src_column, uint32_t (&w)[4])
{
	const SaveWindow win = save_window(row, stride, src_column);
	const uint64_t base = win.byte & ~15ull;
	const SaveQuad p = load4(base), q = load4(base + 16);
	const uint32_t e[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
	const uint32_t at = (uint32_t)(win.byte - base);                        // 4, 8 or 12
	const uint32_t one = 0u - (uint32_t)(at == 4), two = 0u - (uint32_t)(at == 8), three = 0u - (uint32_t)(at == 12);
	uint32_t a[5];
	for(int j = 0; j < 5; ++j){ a[j] = (e[1 + j] & one) | (e[2 + j] & two) | (e[3 + j] & three); }
	if(win.shift == 0){ a[4] = 0u; }
	for(int j = 0; j < 4; ++j){ w[j] = (uint32_t)(((uint64_t)a[j] | ((uint64_t)a[j + 1] << 32)) >> win.shift); }
}

// Unit `unit` (columns 128 unit .. 128 unit + 127) of destination row `row`, from loads of the SOURCE matrix (rows
// src_stride bytes apart, src_bytes in all): w[0..3] are its four words -- destination column first_column + d holds the
// source column of the run that covers d, for d < n; everything below first_column and at and above first_column + n is
// zero (the kernel ORs in what it keeps from memory, copy_keep_mask).  A unit that lies wholly inside
// [first_column, first_column + n) and inside ONE run has its loads requested together -- save_unit_in_run's path where
// its source columns start on a 16-byte boundary of the row, copy_unit_off_boundary's where they do not; every other unit -- the first and the last of a row, one a run ends or begins in -- is walked piece by piece (save_word over
// save_piece), the dword loaded last kept for the next piece.
// load(byte offset) returns the dword there, load4(byte offset) the 16 bytes at a 16-byte boundary.
template <typename LOAD, typename LOAD4>
KWAGE_HD inline void copy_unit_value(LOAD &&load, LOAD4 &&load4, const SaveRun *runs, uint32_t n_runs, uint64_t row, uint64_t src_stride,
                                     uint64_t src_bytes, uint64_t first_column, uint64_t n, uint64_t unit, uint32_t (&w)[4])
{
	const uint64_t c0 = 128*unit, end = first_column + n;
	w[0] = w[1] = w[2] = w[3] = 0u;
	if(c0 >= end || c0 + 128 <= first_column){ return; }
	uint32_t k = save_find_run(runs, n_runs, (uint32_t)(std::max(c0, first_column) - first_column));
	if(c0 >= first_column && c0 + 128 <= end){
		const SaveRun r = runs[k];
		const uint32_t d0 = (uint32_t)(c0 - first_column);
		if((uint64_t)d0 + 128 <= (uint64_t)r.dst_first + r.len){
			const uint64_t src_column = r.src_first + (d0 - r.dst_first);
			if(save_window(row, src_stride, src_column).byte % 16 == 0){ save_unit_in_run(load, load4, row, src_stride, src_column, w); }
			else{ copy_unit_off_boundary(load4, row, src_stride, src_column, w); }
			return;
		}
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
		const uint64_t lo = std::max(c0 + 32u*j, first_column), hi = std::min(c0 + 32u*j + 32, end);
		if(lo < hi){
			w[j] = save_word(load_kept, runs, &k, row, src_stride, src_bytes, (uint32_t)(lo - first_column), (uint32_t)(hi - first_column)) << (lo - (c0 + 32u*j));
		}
	}
}

}  // namespace kwage

#endif
