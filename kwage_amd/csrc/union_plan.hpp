// kwage_amd/csrc/union_plan.hpp -- the host-side planning of the union of columns (union.hip, kwage_group_union_columns):
// the refusals, the (source dword, mask) entries the member lists fold into, where the new columns go in the destination
// (the live insert's rule, insert_plan.hpp plan_insert; within ONE group always the next 16-byte boundary of the row), the
// 16-byte units of a destination row that are written, and -- written ONCE for the kernel and the host -- the value of one
// such unit.  What a unit keeps from memory is the copy's (copy_plan.hpp copy_keep_mask).  Plain functions of plain
// values: no device, no group -- tests/sanitize/union_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_UNION_PLAN_HPP
#define KWAGE_AMD_UNION_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "copy_plan.hpp"
#include "insert_plan.hpp"

namespace kwage {

// One load of a union: dword `dword` of a source row (columns 32 dword .. 32 dword + 31), of which the bits of `mask` are
// members of ONE set -- the set's new column is set in a row where load & mask is nonzero for any entry of the set.  That
// column is bit `bit` (one bit set) of word `word` (0 .. 3) of its 16-byte unit of the destination row: (first + set) %
// 128 says both, whatever the unit.  16 bytes: a lane fetches an entry with one load.  (Where the result goes stands in
// the entry so that a lane walks the entries of ALL the sets of its unit as one stretch of the table, eight at a time,
// whatever the sets' sizes.)
struct UnionEntry { uint32_t dword, mask, word, bit; };

// What a union of n sets into destination columns first .. first + n - 1 does:
//   entries                per set the distinct source dwords of its members, ascending, each with the members' bits; the
//                          sets one behind the other in list order
//   offsets                n + 1: the entries of set j are entries[offsets[j] .. offsets[j + 1]) (CSR)
//   first_unit, units      the 16-byte units of a destination row that are stored: [first_unit, first_unit + units)
struct UnionPlan {
	uint64_t first = 0, n = 0, members = 0, first_unit = 0, units = 0;
	std::vector<UnionEntry> entries;
	std::vector<uint32_t> offsets;
};

// The refusals of kwage_group_union_columns that need no look at a member, in the order the call makes them; dst and src
// may be NULL, set_offsets is read only where it and everything before it passed.  (The pending search is
// KWAGE_ERR_STATE, everything else KWAGE_ERR_ARG.)  dst == src is allowed.
inline int union_refusal(const CopySide *dst, const CopySide *src, bool have_columns, const uint64_t *set_offsets, bool have_first,
                         uint32_t n_sets, bool search_pending)
{
	const char *who = "kwage_group_union_columns";
	if(!dst || !src || !have_columns || !set_offsets || !have_first){
		return fail(KWAGE_ERR_ARG, "%s: NULL %s", who, !dst ? "dst" : !src ? "src" : !have_columns ? "columns" : !set_offsets ? "set_offsets" : "first_column");
	}
	if(n_sets == 0){ return fail(KWAGE_ERR_ARG, "%s: n_sets is 0", who); }
	if(set_offsets[0] != 0){ return fail(KWAGE_ERR_ARG, "%s: set_offsets[0] is %llu, not 0", who, (unsigned long long)set_offsets[0]); }
	for(uint32_t j = 0; j < n_sets; ++j){
		if(set_offsets[j + 1] < set_offsets[j]){
			return fail(KWAGE_ERR_ARG, "%s: set_offsets decreases at set %u: %llu after %llu", who, j, (unsigned long long)set_offsets[j + 1], (unsigned long long)set_offsets[j]);
		}
		if(set_offsets[j + 1] == set_offsets[j]){ return fail(KWAGE_ERR_ARG, "%s: set %u is empty", who, j); }
	}
	if(dst->ctx != src->ctx){ return fail(KWAGE_ERR_ARG, "%s: the groups belong to different contexts", who); }
	if(dst->sparse || src->sparse){ return fail(KWAGE_ERR_ARG, "%s: a sparse group takes part in no union", who); }
	const kwage_params &a = dst->params, &b = src->params;
	if(a.kmer_len != b.kmer_len){ return fail(KWAGE_ERR_ARG, "%s: kmer_len differs: dst %u, src %u", who, a.kmer_len, b.kmer_len); }
	if(a.num_hash != b.num_hash){ return fail(KWAGE_ERR_ARG, "%s: num_hash differs: dst %u, src %u", who, a.num_hash, b.num_hash); }
	if(a.log_2_filter_len != b.log_2_filter_len){ return fail(KWAGE_ERR_ARG, "%s: log_2_filter_len differs: dst %u, src %u", who, a.log_2_filter_len, b.log_2_filter_len); }
	if(a.hash_func != b.hash_func){ return fail(KWAGE_ERR_ARG, "%s: hash_func differs: dst %d, src %d", who, (int)a.hash_func, (int)b.hash_func); }
	if(search_pending){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); }
	return KWAGE_OK;
}

// More list entries than the entry table's 32-bit offsets count (the entries are at most as many as the members).
inline int union_count_refusal(uint64_t members)
{
	if(members > 0xFFFFFFFFull){ return fail(KWAGE_ERR_ARG, "kwage_group_union_columns: %llu members do not fit an entry table", (unsigned long long)members); }
	return KWAGE_OK;
}

// The member lists (union_refusal passed) checked, folded and placed.  Refused (KWAGE_ERR_ARG, the plan's tables empty),
// in this order: a member at or beyond the source's span, a pad or retired column of src_valid[] (a bit per column, LSB
// first; the first offender in list order), more than 2^32 - 1 members, more sets than the destination's row holds behind
// where they land (plan_insert).  A member repeated within a set is folded; a member may stand in several sets.
// same_group: the new columns start at the next 16-byte boundary of the row ALSO behind an open tail, so every unit
// written lies wholly above everything a member can lie in.
inline int plan_union(const uint64_t *columns, const uint64_t *set_offsets, uint32_t n_sets, uint64_t src_span, const uint8_t *src_valid, bool same_group,
                      uint64_t dst_next_byte, bool dst_tail_open, uint64_t dst_tail_column, uint64_t dst_stride, UnionPlan &plan)
{
	const char *who = "kwage_group_union_columns";
	plan.entries.clear();
	plan.offsets.clear();
	const uint64_t members = set_offsets[n_sets];
	for(uint64_t i = 0; i < members; ++i){
		const uint64_t c = columns[i];
		if(c >= src_span){ return fail(KWAGE_ERR_ARG, "%s: column %llu is at or beyond the span %llu", who, (unsigned long long)c, (unsigned long long)src_span); }
		if(!((src_valid[c/8] >> (c%8)) & 1)){ return fail(KWAGE_ERR_ARG, "%s: column %llu is a pad or retired column", who, (unsigned long long)c); }
	}
	int rc = union_count_refusal(members);
	if(rc){ return rc; }
	uint64_t first = 0;
	if((rc = plan_insert(dst_next_byte, dst_tail_open && !same_group, dst_tail_column, dst_stride, n_sets, &first))){ return rc; }
	plan.offsets.reserve((size_t)n_sets + 1);
	plan.offsets.push_back(0u);
	std::vector<uint64_t> sorted;
	for(uint32_t j = 0; j < n_sets; ++j){
		sorted.assign(columns + set_offsets[j], columns + set_offsets[j + 1]);
		std::sort(sorted.begin(), sorted.end());
		const size_t begin = plan.entries.size();
		const uint32_t at = (uint32_t)((first + j) % 128);
		for(uint64_t c : sorted){
			if(plan.entries.size() == begin || plan.entries.back().dword != (uint32_t)(c/32)){ plan.entries.push_back(UnionEntry{(uint32_t)(c/32), 0u, at/32, 1u << (at%32)}); }
			plan.entries.back().mask |= 1u << (c%32);
		}
		plan.offsets.push_back((uint32_t)plan.entries.size());
	}
	plan.first = first;
	plan.n = n_sets;
	plan.members = members;
	plan.first_unit = first/128;
	plan.units = (first + n_sets + 127)/128 - plan.first_unit;
	return KWAGE_OK;
}

constexpr int UNION_LOADS = 8;      // source dwords a lane requests together

// On the device: nothing is moved across this point by the instruction scheduler, so the loads written before it are all
// requested before the first wait for one of them.  Nothing on the host.
#if defined(__HIP_DEVICE_COMPILE__)
#define KWAGE_UNION_ISSUED() __builtin_amdgcn_sched_barrier(0)
#else
#define KWAGE_UNION_ISSUED() ((void)0)
#endif

// Unit `unit` (columns 128 unit .. 128 unit + 127) of destination row `row`, from loads of the SOURCE matrix (rows
// src_stride bytes apart): w[0..3] are its four words.  With shift = first_column - 128 first_unit, bit d of the unit is
// set where any entry of set 128 (unit - first_unit) + d - shift has load(dword) & mask nonzero; everything below
// first_column and at and above first_column + n is zero (the kernel ORs in what it keeps from memory, copy_keep_mask).
// The sets of a unit are consecutive, so their entries are ONE stretch of the table: it is walked UNION_LOADS entries at
// a time -- the entries fetched together, then their source dwords requested together, then the tests.  The last round
// repeats the stretch's last entry in place of what lies behind it: the OR does not mind, and nothing depends on a count.
// entry(i) returns entries[i], load(byte offset) the source dword there.
template <typename ENTRY, typename LOAD>
KWAGE_HD inline void union_unit_value(ENTRY &&entry, LOAD &&load, const uint32_t *offsets, uint64_t row, uint64_t src_stride,
                                      uint64_t first_column, uint64_t n, uint64_t unit, uint32_t (&w)[4])
{
	const uint64_t c0 = 128*unit, end = first_column + n;
	w[0] = w[1] = w[2] = w[3] = 0u;
	if(c0 >= end || c0 + 128 <= first_column){ return; }
	const uint64_t set_lo = std::max(c0, first_column) - first_column, set_hi = std::min(c0 + 128, end) - first_column;
	const uint32_t e_lo = offsets[set_lo], e_hi = offsets[set_hi];
	if(e_lo >= e_hi){ return; }
	const uint64_t row_byte = row*src_stride;
#if defined(__clang__)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
#endif
	for(uint64_t e = e_lo; e < e_hi; e += UNION_LOADS){
		UnionEntry en[UNION_LOADS];
		uint32_t v[UNION_LOADS];
		for(int i = 0; i < UNION_LOADS; ++i){ en[i] = entry(std::min<uint64_t>(e + (uint64_t)i, (uint64_t)e_hi - 1)); }
		KWAGE_UNION_ISSUED();
		for(int i = 0; i < UNION_LOADS; ++i){ v[i] = load(row_byte + 4ull*en[i].dword); }
		KWAGE_UNION_ISSUED();
		for(int i = 0; i < UNION_LOADS; ++i){
			const uint32_t hit = (v[i] & en[i].mask) != 0u ? en[i].bit : 0u;
			// (no indexed write: the words stay in registers)
			w[0] |= en[i].word == 0 ? hit : 0u; w[1] |= en[i].word == 1 ? hit : 0u; w[2] |= en[i].word == 2 ? hit : 0u; w[3] |= en[i].word == 3 ? hit : 0u;
		}
	}
}

}  // namespace kwage

#endif
