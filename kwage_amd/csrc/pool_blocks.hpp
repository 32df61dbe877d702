// kwage_amd/csrc/pool_blocks.hpp -- what the synchronous calls of topk.hip, topk_merge.hip, scores.hip, presence.hip and
// filterset.hip share: the refusals every search starts with (search_check); the device blocks of one call, taken from
// the context's batch pool and handed back when the call ends; the tail every entry point ends through (settle); the
// events of a timed call and the timed section; the k-mer stage into blocks of the call.
#ifndef KWAGE_AMD_POOL_BLOCKS_HPP
#define KWAGE_AMD_POOL_BLOCKS_HPP

#include <vector>

#include "engine_state.hpp"

namespace kwage {

// What every search of a batch in a group refuses first.
inline int search_check(const kwage_group *g, const kwage_batch *b)
{
	if(!g->finalized){ return fail(KWAGE_ERR_STATE, "kwage_group_finalize() must be called before searching"); }
	if(b->ctx != g->ctx){ return fail(KWAGE_ERR_ARG, "batch and group belong to different contexts"); }
	return KWAGE_OK;
}

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

// An error return may leave kernels of the call queued: nothing of it may still run when its PoolBlocks hands the
// device memory back to the pool (the destructor that follows).  Returns rc.
inline int settle(kwage_ctx *ctx, int rc)
{
	if(rc && ctx){
		(void)hipStreamSynchronize(ctx->stream);
		(void)hipGetLastError();
	}
	return rc;
}

// N events, created on demand (a call that is not timed creates none) and destroyed with the holder.
template <int N>
struct Events {
	hipEvent_t ev[N] = {};
	~Events() { for(hipEvent_t e : ev){ if(e){ (void)hipEventDestroy(e); } } }
	int create()
	{
		for(hipEvent_t &e : ev){ HIP_TRY(hipEventCreate(&e)); }
		return KWAGE_OK;
	}
};

// What body() queues on s, then the wait for s.  timing: between two events, whose distance goes to *ms.
template <typename Body>
int timed_section(bool timing, hipStream_t s, float *ms, Body &&body)
{
	int rc;
	Events<2> ev;
	if(timing && (rc = ev.create())){ return rc; }
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[0], s)); }
	if((rc = body())){ return rc; }
	if(timing){ HIP_TRY(hipEventRecord(ev.ev[1], s)); }
	HIP_TRY(hipStreamSynchronize(s));
	if(timing){ HIP_TRY(hipEventElapsedTime(ms, ev.ev[0], ev.ev[1])); }
	return KWAGE_OK;
}

// What the k-mer stage of a call leaves in its blocks: the row indices, and per query (batch order) the k-mer count,
// the floor and -- where asked for -- one more word for the caller; the 8-byte aligned counter of row indices a sparse
// group does not hold.
struct KmerBlocks {
	uint32_t *rows = nullptr, *nkmer = nullptr, *qthr = nullptr, *extra = nullptr;
	unsigned long long *missing = nullptr;
};

// The k-mer stage of batch b (layout L) for group g on stream s, not waited for: distinct canonical k-mers, their row
// indices (a sparse group's: positions in its row list) and the floor (unsigned)(threshold * n) of every query.
// `missing` is cleared for a sparse group, which counts into it, and where clear_missing asks for it.  timed: null, or
// two events recorded before and behind the queued stage.  KWAGE_ERR_ARG for a query of 2^32 rows and more.
inline int kmer_prologue(const kwage_group *g, kwage_batch *b, const KmerLayout *L, float threshold, bool extra, bool clear_missing,
                         hipEvent_t *timed, PoolBlocks &blocks, hipStream_t s, KmerBlocks *out)
{
	int rc;
	const uint32_t n = b->n, nh = g->params.num_hash, n1 = std::max<uint32_t>(n, 1);
	if(L->max_pos*nh > 0xFFFFFFFFull){
		return fail(KWAGE_ERR_ARG, "a query of %llu k-mer positions x %u hash functions exceeds 2^32 rows", (unsigned long long)L->max_pos, nh);
	}
	KmerBlocks k;
	if((rc = blocks.take(std::max<uint64_t>(L->total_pos*nh, 1)*sizeof(uint32_t), &k.rows))){ return rc; }
	if((rc = blocks.take((uint64_t)n1*sizeof(uint32_t)*(extra ? 3 : 2) + 16, &k.nkmer))){ return rc; }
	k.qthr = k.nkmer + n1;
	k.extra = extra ? k.qthr + n1 : nullptr;
	k.missing = (unsigned long long*)(((uintptr_t)(k.qthr + (extra ? 2 : 1)*(size_t)n1) + 7) & ~(uintptr_t)7);
	if(clear_missing || (n && g->d_row_map)){ HIP_TRY(hipMemsetAsync(k.missing, 0, sizeof(unsigned long long), s)); }
	if(timed){ HIP_TRY(hipEventRecord(timed[0], s)); }
	if(n){
		unsigned long long *d_tables = nullptr;
		if(L->table_slots){
			if((rc = blocks.take(L->table_slots*sizeof(uint64_t), &d_tables))){ return rc; }
			HIP_TRY(hipMemsetAsync(d_tables, 0xFF, L->table_slots*sizeof(uint64_t), s));
		}
		const KmerStageOut o = {k.rows, nullptr, k.nkmer, k.qthr, d_tables};
		if((rc = launch_kmer_kernels(g->params, b, L, threshold, 0, o, s))){ return rc; }
		if(g->d_row_map && (rc = launch_remap_rows(g, n, L, k.rows, k.nkmer, k.missing, s))){ return rc; }
	}
	if(timed){ HIP_TRY(hipEventRecord(timed[1], s)); }
	*out = k;
	return KWAGE_OK;
}

// The k-mer stage of a search that writes into the caller's memory: kmer_prologue, then -- waited for -- the refusal of
// a sparse group made for other queries, before anything is written; then the queued copy of the k-mer counts, final
// here, to nkmer_dev (null: none), ahead of what the caller queues next.
inline int kmer_prologue_checked(const kwage_group *g, kwage_batch *b, const KmerLayout *L, float threshold, void *nkmer_dev,
                                 PoolBlocks &blocks, hipStream_t s, KmerBlocks *out)
{
	int rc;
	if((rc = kmer_prologue(g, b, L, threshold, false, false, nullptr, blocks, s, out))){ return rc; }
	if(b->n && g->d_row_map){
		unsigned long long missing = 0;
		HIP_TRY(hipMemcpyAsync(&missing, out->missing, sizeof(missing), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if(missing){ return fail_missing_rows(missing); }
	}
	if(b->n && nkmer_dev){ HIP_TRY(hipMemcpyAsync(nkmer_dev, out->nkmer, (size_t)b->n*sizeof(uint32_t), hipMemcpyDefault, s)); }
	return KWAGE_OK;
}

}  // namespace kwage

#endif
