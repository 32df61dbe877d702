// kwage_amd/csrc/insert_plan.hpp -- the host-side planning of the live insert (insert.hip): where the columns of an insert
// go, what the insert kernel's launch covers, and which (word, mask) pairs a retire clears.  Plain functions of plain
// values: no device, no group -- tests/sanitize/insert_sanitize.cpp drives them under the sanitizers.
#ifndef KWAGE_AMD_INSERT_PLAN_HPP
#define KWAGE_AMD_INSERT_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

#include "internal.h"

namespace kwage {

// The reservation rule.  A group whose last reservation was an insert has an OPEN tail: the next insert continues at the
// very next column (tail_column; next_byte == ceil(tail_column/8)).  Otherwise -- a fresh group, or a file / host / random
// block was reserved since, which closes the tail -- it starts at the next 16-byte boundary of the row like every other
// block.  Nothing is changed here: the caller commits first_column + n as the new tail once every other check has passed.
inline int plan_insert(uint64_t next_byte, bool tail_open, uint64_t tail_column, uint64_t stride, uint64_t n, uint64_t *first_column)
{
	if(n == 0){ return fail(KWAGE_ERR_ARG, "cannot insert 0 filters"); }
	const uint64_t first = tail_open ? tail_column : (next_byte + 15)/16*16*8;
	if(first > 8*stride || n > 8*stride - first){
		return fail(KWAGE_ERR_ARG, "group capacity exceeded: need column %llu of a row of %llu",
		            (unsigned long long)(first + n), (unsigned long long)(8*stride));
	}
	*first_column = first;
	return KWAGE_OK;
}

// What the insert kernel's launch covers in a row: destination words [word_first, word_last] of 32 columns, of which the
// first keeps its bits below `keep_bits` from memory; the kernel's tiles start at word_base, the 16-byte boundary at or
// below word_first, and the filters sit `shift` columns above it.
struct InsertSpan {
	uint64_t word_base, word_first, word_last;
	uint32_t keep_bits, shift;
};
inline InsertSpan insert_span(uint64_t first_column, uint64_t n)
{
	InsertSpan s;
	s.word_first = first_column/32;
	s.word_last = (first_column + n - 1)/32;
	s.word_base = s.word_first & ~3ull;
	s.keep_bits = (uint32_t)(first_column % 32);
	s.shift = (uint32_t)(first_column - 32*s.word_base);      // 0 .. 127
	return s;
}

// A retire's columns folded into distinct (32-bit word of a row, mask) pairs, ascending: one thread per (row, pair) clears
// its mask, so two columns of one word never meet.  Columns may repeat; each must lie below the span and be a real column
// of valid[] (the group's host valid mask, a bit per column, LSB first), else KWAGE_ERR_ARG.  *distinct = columns named.
struct RetirePair { uint64_t word; uint32_t mask; uint32_t pad; };
inline int plan_retire(const uint8_t *valid, uint64_t span, const uint64_t *columns, uint64_t n, std::vector<RetirePair> &pairs, uint64_t *distinct)
{
	pairs.clear();
	*distinct = 0;
	for(uint64_t i = 0; i < n; ++i){
		const uint64_t c = columns[i];
		if(c >= span){ return fail(KWAGE_ERR_ARG, "kwage_group_retire_columns: column %llu is at or beyond the span %llu", (unsigned long long)c, (unsigned long long)span); }
		if(!((valid[c/8] >> (c%8)) & 1)){ return fail(KWAGE_ERR_ARG, "kwage_group_retire_columns: column %llu is a pad column", (unsigned long long)c); }
	}
	std::vector<uint64_t> cols(columns, columns + n);
	std::sort(cols.begin(), cols.end());
	cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
	for(uint64_t c : cols){
		if(pairs.empty() || pairs.back().word != c/32){ pairs.push_back(RetirePair{c/32, 0u, 0u}); }
		pairs.back().mask |= 1u << (c%32);
	}
	*distinct = cols.size();
	return KWAGE_OK;
}

}  // namespace kwage

#endif
