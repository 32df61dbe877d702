// kwage_amd/csrc/pool_blocks.hpp -- device blocks of one synchronous call, taken from the context's batch pool and
// handed back when the call ends.  Shared by topk.hip, topk_merge.hip, scores.hip and filterset.hip.  The caller synchronises the stream before
// the object goes out of scope on an error path: nothing queued by the call may still read the blocks.
#ifndef KWAGE_AMD_POOL_BLOCKS_HPP
#define KWAGE_AMD_POOL_BLOCKS_HPP

#include <vector>

#include "engine_state.hpp"

namespace kwage {

struct PoolBlocks {
	DevPool *pool;
	std::vector<DevPool::Block> held;
	explicit PoolBlocks(DevPool *p) : pool(p) {}
	~PoolBlocks() { for(const DevPool::Block &b : held){ pool->give(b.p, b.cap); } }
	PoolBlocks(const PoolBlocks&) = delete;
	PoolBlocks &operator=(const PoolBlocks&) = delete;
	template <typename T>
	int take(uint64_t bytes, T **out)
	{
		void *p = nullptr;
		uint64_t cap = 0;
		HIP_TRY(pool->take(bytes, &p, &cap));
		held.push_back(DevPool::Block{p, cap});
		*out = (T*)p;
		return KWAGE_OK;
	}
};

}  // namespace kwage

#endif
