// kwage_amd/csrc/fold_plan.hpp -- the host-side planning of the fold (fold.hip, kwage_group_fold): the refusals, the
// 16-byte units of a row that are read and written, the items and the grid, the loads per item and pass, the byte counts
// of the stats, and -- written ONCE for the kernel and the host -- where an item lies and how its 16 bytes are made from
// loads.  Plain functions of plain values: no device, no group -- tests/sanitize/fold_sanitize.cpp drives them under the
// sanitizers.
#ifndef KWAGE_AMD_FOLD_PLAN_HPP
#define KWAGE_AMD_FOLD_PLAN_HPP

#include <algorithm>
#include <cstdint>

#include "internal.h"

#if defined(__HIPCC__)
#define KWAGE_HD __host__ __device__
#else
#define KWAGE_HD
#endif

namespace kwage {

constexpr uint32_t FOLD_THREADS = 256;          // lanes of a workgroup (fold_kernels.hpp says why)
constexpr uint32_t FOLD_LOADS_IN_FLIGHT = 8;    // 16-byte loads a lane has requested before it waits for any: the gather kernels' shape

// The fold of a group of 2^log_2_before rows to 2^log_2_after rows, rows `stride` bytes apart in both matrices:
//   an ITEM is one 16-byte unit of one destination row: item = row * units_per_row + unit.  Its 2^f sources
//   (f = log_2_before - log_2_after) are the same unit of the source rows row + j * 2^log_2_after: src_step bytes apart
//   J                      log2 of the loads per item and pass, min(f, 3): a lane takes items_per_lane = 8 >> J items of a
//                          chunk at a time and ORs `passes` = 2^(f - J) rounds of 2^J loads into each
//   chunks                 an item belongs to chunk item / (FOLD_THREADS * items_per_lane); the persistent grid of at most
//                          8 workgroups per compute unit strides over the chunks
struct FoldPlan {
	uint32_t log_2_before = 0, log_2_after = 0, f = 0, J = 0;
	uint32_t items_per_lane = 0, passes = 0;
	uint64_t units_per_row = 0, dst_rows = 0, items = 0, src_step = 0, chunks = 0;
	uint32_t grid = 0;
	uint64_t bytes_read = 0, bytes_written = 0;
};

// The refusals of kwage_group_fold, in the order the call makes them -- all before anything is allocated.
inline int fold_refusal(bool have_src, bool have_out, bool sparse, uint32_t log_2_before, uint32_t log_2_after, bool search_pending)
{
	const char *who = "kwage_group_fold";
	if(!have_src || !have_out){ return fail(KWAGE_ERR_ARG, "%s: NULL %s", who, have_src ? "out" : "group"); }
	if(sparse){ return fail(KWAGE_ERR_ARG, "%s: a sparse group is not folded", who); }
	if(log_2_after >= log_2_before){
		return fail(KWAGE_ERR_ARG, "%s: log_2_filter_len %u is not below the group's %u", who, log_2_after, log_2_before);
	}
	if(search_pending){ return fail(KWAGE_ERR_STATE, "%s: a search is pending on this context", who); }
	return KWAGE_OK;
}

// row_bytes: kwage_group_row_bytes of the source (ceil(span / 8)); ncu: compute units of the device.  A span of 0 has no
// item: nothing is launched (grid == 0).
inline FoldPlan plan_fold(uint32_t log_2_before, uint32_t log_2_after, uint64_t row_bytes, uint64_t stride, int ncu)
{
	FoldPlan p;
	p.log_2_before = log_2_before;
	p.log_2_after = log_2_after;
	p.f = log_2_before - log_2_after;
	p.J = std::min<uint32_t>(p.f, 3);
	p.items_per_lane = FOLD_LOADS_IN_FLIGHT >> p.J;
	p.passes = 1u << (p.f - p.J);
	p.units_per_row = (row_bytes + 15)/16;
	p.dst_rows = 1ull << log_2_after;
	p.items = p.dst_rows*p.units_per_row;
	p.src_step = p.dst_rows*stride;
	const uint64_t per_chunk = (uint64_t)FOLD_THREADS*p.items_per_lane;
	p.chunks = (p.items + per_chunk - 1)/per_chunk;
	p.grid = (uint32_t)std::min<uint64_t>(p.chunks, (uint64_t)std::max(ncu, 1)*8);
	p.bytes_read = (p.items << p.f)*16;
	p.bytes_written = p.items*16;
	return p;
}

// The i-th item (i < items_per_lane) of lane `lane` in chunk `chunk`: consecutive lanes take consecutive items, so a
// wave's loads of one source row and its store are contiguous wherever a row has 64 units and more.
KWAGE_HD inline uint64_t fold_chunk_item(uint64_t chunk, uint32_t items_per_lane, uint32_t i, uint32_t lane)
{
	return (chunk*items_per_lane + i)*FOLD_THREADS + lane;
}

// Where an item lies: its destination row and unit, and `byte` -- the offset of the unit in the destination matrix, which
// is also the offset of its FIRST source unit in the source matrix (the same row number, the same stride); source j lies
// at byte + j * src_step.  All in 64 bits: a matrix of 2^23 rows of 12544 bytes has offsets beyond 2^36.  One division
// (of 32-bit values wherever the item number has 32 bits: units_per_row always has, the stride is below 2^35).
struct FoldItem { uint64_t row, unit, byte; };
KWAGE_HD inline FoldItem fold_item(uint64_t item, uint64_t units_per_row, uint64_t stride)
{
	FoldItem it;
	if((item >> 32) == 0){ it.row = (uint32_t)item/(uint32_t)units_per_row; }
	else{ it.row = item/units_per_row; }
	it.unit = item - it.row*units_per_row;
	it.byte = it.row*stride + 16*it.unit;
	return it;
}

// An item's 16 bytes, one load after the other: the path of a chunk that is not whole (the last one; a matrix of fewer
// items than a workgroup takes at a time), and the host's restatement of every item.  load4(byte offset) returns the 16
// bytes at a 16-byte boundary of the source matrix.
struct FoldQuad { uint32_t x, y, z, w; };
template <typename LOAD4>
KWAGE_HD inline FoldQuad fold_item_value(LOAD4 &&load4, uint64_t byte, uint64_t src_step, uint64_t n_src)
{
	FoldQuad acc = {0u, 0u, 0u, 0u};
	for(uint64_t j = 0; j < n_src; ++j, byte += src_step){
		const FoldQuad q = load4(byte);
		acc.x |= q.x; acc.y |= q.y; acc.z |= q.z; acc.w |= q.w;
	}
	return acc;
}

}  // namespace kwage

#endif
