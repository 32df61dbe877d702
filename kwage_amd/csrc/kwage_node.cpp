// kwage_amd/csrc/kwage_node.cpp -- `kwage_node`: the kwage command line on every GPU of a node, ONE PROCESS PER GPU, the
// per-GPU hit lists concatenated on rank 0 by a variable-length gather over RCCL.
//
// Same options, same database files, same CSV / JSON bytes as `kwage` (and therefore as the reference): the option
// parser, query readers, hit records and report writers are the ones `kwage` uses (cli_common.hpp), so the two programs
// cannot drift apart.  What differs is how a node's GPUs are used:
//
//   kwage  (KWAGE_DEVICES=all)   one process, a host thread + context per GPU, hit lists merged in host memory
//   kwage_node                   one process per GPU (forked before anything touches a device), the sample (column)
//                                axis sharded by whole files (a file belongs to the rank that owns its middle column,
//                                the rule of kwage's node mode and of kwage_amd.distributed.partition_files), queries
//                                replicated, and per query batch ONE exchange:  every rank searches its groups with
//                                kwage_search_device_append_submit (all groups append to one device list, the records
//                                carry GLOBAL column numbers), ncclAllGather of the record counts, one grouped
//                                ncclSend / ncclRecv of the records in exact sizes to rank 0 (RCCL has no gatherv),
//                                rank 0 maps columns back to (file, column in file) and writes the report.
//
// This is the reference's only parallel axis (OpenMP over database files, kwage.cpp:76-87) and its critical-section
// merge (kwage.cpp:154-177) at node scale, as BASELINE's north star words it.  The library itself stays free of RCCL:
// only this program links it.  No row data ever crosses xGMI.
//
//   KWAGE_NODE_RANKS    number of ranks (default: the number of visible devices); rank r uses device r
//   KWAGE_NODE_PLAN     1: print the plan (groups, every rank's files, global column bases; under KWAGE_MAX_GROUP_BYTES also
//                       every rank's passes) as JSON and stop; no device is touched or counted -- the number of ranks must
//                       come from KWAGE_NODE_RANKS
//   KWAGE_NODE_STATS    1: rank 0 reports on stderr what the search phase took: wall, sum of gather-kernel time, exchange, filing
//   KWAGE_NODE_REHEARSE 1: rehearsal on a machine with fewer GPUs than ranks -- every rank uses device 0 and the records
//                       travel through a shared host segment instead of RCCL (which refuses two ranks on one device).
//                       The searches still run on the GPU; sharding, global numbering, gather and report are the same
//                       code.  For tests on one-GPU boxes, not for production.
//   KWAGE_EARLY_EXIT, KWAGE_BATCH_BASES, KWAGE_MAX_GROUP_BYTES   as for kwage
//   KWAGE_NODE_COMM_TIMEOUT_S   how long a rank waits for the communicator to come up (default 120 s): a rank whose peers never
//                       arrive exits non-zero instead of waiting forever, and the parent ends the others
// A database that does not fit its ranks' HBM is searched in PASSES, as kwage does it (kwage_main.cpp: units of whole files
// packed into what is free; the query sources are read once per pass; results are additive): every rank plans every
// rank's passes from the file headers and the ranks' budgets (one all-gather), so all of them make the same number of
// exchanges -- a rank whose files are done contributes empty lists.
#include "node_common.hpp"

namespace {

// One rank's software pipeline over query batches (what kwage_amd/distributed.py's StepPipeline is for the Python host).
// A STEP = one query batch against every group this rank holds; all of a step's searches append to ONE device list
// (kwage_search_device_append_submit: the first search of a step zeroes the list's counter in stream order, every record
// carries a GLOBAL column number).  The context runs two searches at a time: begin() queues a step's searches, finish()
// completes the oldest step, feeding the slots as they come free -- so the next batch's first gather kernels are already
// running while the finished batch's hits are exchanged over RCCL and filed on rank 0.  THREE lists rotate: batch i+2 is
// queued before batch i is exchanged (the collective's kernel waits for wave slots behind the running gather kernel, and
// the device must have the next gather kernel queued while the host waits for it).
struct HitList {
	uint64_t *d_count = nullptr;         // the list's record counter (what the gather kernels add to)
	kwage_hit *d_hits = nullptr;
	uint64_t cap = 0;
};

struct Step {
	QueryBatch q;
	kwage_batch *b = nullptr;
	int list = 0;
	size_t searches = 0, done = 0;
	uint64_t n = 0;                      // records in the list (the running total the last search leaves)
	double kernel_ms = 0;
	map<uint32_t, vector<uint32_t> > nk; // rank 0: num_query_kmer per k-mer length, taken from this rank's own searches
	Findings *found = nullptr;
};

struct RankPipeline {
	kwage_ctx *ctx;
	vector<Unit> *units = nullptr;       // what is resident in the current pass
	int rank;
	float threshold;
	uint32_t flags;
	HitList lists[3];
	uint32_t *d_nk = nullptr;            // where a search leaves num_query_kmer for the host (rank 0)
	uint64_t nk_cap = 0;
	struct Todo { Step *step; size_t gi; bool first; };
	struct Flying { kwage_pending *p; Step *step; size_t gi; };
	deque<Todo> todo;
	deque<Flying> flying;
	int next_list = 0;

	RankPipeline(kwage_ctx *c, int r, float t, uint32_t f) : ctx(c), rank(r), threshold(t), flags(f)
	{
		for(HitList &l : lists){
			l.cap = 1u << 18;
			NODE_HIP(hipMalloc((void**)&l.d_count, sizeof(uint64_t)));
			NODE_HIP(hipMemset(l.d_count, 0, sizeof(uint64_t)));
			NODE_HIP(hipMalloc((void**)&l.d_hits, l.cap*sizeof(kwage_hit)));
		}
	}
	~RankPipeline()
	{
		for(Flying &f : flying){ uint64_t n = 0; (void)kwage_search_device_collect(f.p, &n, nullptr, nullptr); }
		for(HitList &l : lists){ (void)hipFree(l.d_count); (void)hipFree(l.d_hits); }
		if(d_nk){ (void)hipFree(d_nk); }
	}
	void submit(const Todo &t)
	{
		Unit &u = (*units)[t.gi];
		HitList &l = lists[t.step->list];
		kwage_pending *p = nullptr;
		check(kwage_search_device_append_submit(u.mine, t.step->b, threshold, flags | KWAGE_SEARCH_TIMING, l.d_hits, l.cap, l.d_count,
		                                        (uint32_t)u.base, t.first ? 1 : 0, &p));
		flying.push_back(Flying{p, t.step, t.gi});
	}
	void pump() { while(!todo.empty() && flying.size() < 2){ submit(todo.front()); todo.pop_front(); } }
	void collect_oldest()
	{
		Flying f = flying.front();
		flying.pop_front();
		Step *st = f.step;
		const uint32_t k = (*units)[f.gi].kmer_len;
		// rank 0 files the hits and needs num_query_kmer of every query: it comes with the search (one device-to-host copy
		// per distinct k-mer length and batch), not from a k-mer stage of its own
		const bool want_nk = (rank == 0) && st->q.size() && !st->nk.count(k);
		if(want_nk && st->q.size() > nk_cap){
			if(d_nk){ (void)hipFree(d_nk); d_nk = nullptr; }
			nk_cap = st->q.size() + st->q.size()/4;
			NODE_HIP(hipMalloc((void**)&d_nk, nk_cap*sizeof(uint32_t)));
		}
		uint64_t n = 0;
		float ms = 0;
		check(kwage_search_device_collect(f.p, &n, want_nk ? d_nk : nullptr, &ms));
		if(want_nk){
			vector<uint32_t> &nk = st->nk[k];
			nk.resize(st->q.size());
			NODE_HIP(hipMemcpy(nk.data(), d_nk, nk.size()*sizeof(uint32_t), hipMemcpyDeviceToHost));
		}
		st->n = n;
		st->kernel_ms += ms;
		++st->done;
	}
	// Wait for `stream` (the exchange's) WITHOUT leaving the device unfed: a collective queued behind a running gather
	// kernel can take as long as that kernel, and only two searches are queued at a time -- so while the exchange is
	// pending, searches that have finished are collected and the step's next ones submitted.
	// (No sleeping poll: the host always BLOCKS on something that has to complete anyway -- the oldest search in flight while
	// there is one (its collection frees a slot for the step's next search), the exchange's stream itself otherwise.  Filing
	// a batch a kernel's length later costs nothing: it happens beside the following batches' searches.)
	void wait_feeding(hipStream_t stream)
	{
		for(;;){
			const hipError_t e = hipStreamQuery(stream);
			if(e == hipSuccess){ return; }
			(void)hipGetLastError();
			if(e != hipErrorNotReady){ throw string("hipStreamQuery failed: ") + hipGetErrorString(e); }
			if(flying.empty()){ NODE_HIP(hipStreamSynchronize(stream)); return; }
			collect_oldest();
			pump();
		}
	}
	void begin(Step *st)
	{
		st->list = next_list;
		next_list = (next_list + 1) % 3;
		check(kwage_batch_create(ctx, st->q.bases.data(), st->q.offsets.data(), (uint32_t)st->q.size(), &st->b));
		bool first = true;
		for(size_t ui = 0; ui < units->size(); ++ui){
			todo.push_back(Todo{st, ui, first});
			first = false;
			++st->searches;
		}
		// (a rank with nothing resident in this pass still takes part in the exchange: an empty list)
		if(st->searches == 0){ NODE_HIP(hipMemset(lists[st->list].d_count, 0, sizeof(uint64_t))); }
		pump();
	}
	// Complete every search of `st` (the oldest open step).  A list that outgrew its buffer is redone after growing it.
	void finish(Step *st)
	{
		while(st->done < st->searches){ collect_oldest(); pump(); }
		HitList &l = lists[st->list];
		if(st->n > l.cap){
			while(!flying.empty()){ collect_oldest(); }       // the next step's searches write the OTHER list: let them finish
			while(st->n > l.cap){
				(void)hipFree(l.d_hits);
				l.cap = st->n + st->n/4;
				NODE_HIP(hipMalloc((void**)&l.d_hits, l.cap*sizeof(kwage_hit)));
				st->done = 0;
				st->kernel_ms = 0;
				bool first = true;
				for(size_t ui = 0; ui < units->size(); ++ui){
					submit(Todo{st, ui, first});
					first = false;
					collect_oldest();
				}
			}
			pump();
		}
	}
};

int run_rank(int rank, int n_ranks, Bootstrap *boot, const Cli &cli, const vector<string> &db_paths, Rehearsal *rehearsal)
{
	return guarded([&]() -> int {
		const time_t started = time(nullptr);
		ofstream fout;
		if(rank == 0 && !open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;

		// ---- headers (every rank) and metadata (rank 0, read on first use) of every database file ---------------------
		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, rank == 0 ? &infos : nullptr, rank == 0);
		vector<NodeGroup> groups = plan_groups(files, n_ranks);
		// where every file's columns begin in the global numbering (ascending: groups, ranks and files are numbered in order)
		vector<ColumnBlock> blocks;
		for(const NodeGroup &g : groups){
			for(size_t r = 0; r < (size_t)n_ranks; ++r){
				for(size_t f = 0; f < g.share[r].files.size(); ++f){
					blocks.push_back(ColumnBlock{g.base[r] + g.share[r].first_column[f], g.share[r].files[f], g.params.kmer_len});
				}
			}
		}

		// ---- this rank's device, its communicator, its matrices ---------------------------------------------------------
		kwage_ctx *ctx = nullptr;
		check(kwage_init(rehearsal ? 0 : rank, &ctx));
		one_shot_placement(ctx);
		ncclComm_t comm = nullptr;
		hipStream_t stream;
		NODE_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		if(!rehearsal){ comm = node_comm_init(rank, n_ranks, boot); }

		// ---- the exchange's buffers: every rank's count, rank 0's gathered list (device + pinned host) ------------------
		const uint32_t flags = env_u64("KWAGE_EARLY_EXIT", 1) ? KWAGE_SEARCH_EARLY_EXIT : 0u;
		const uint64_t max_batch_bases = env_u64("KWAGE_BATCH_BASES", 64ull << 20);
		const bool stats = env_u64("KWAGE_NODE_STATS", 0) != 0;
		uint64_t all_cap = 0, host_cap = 0;
		uint64_t *d_counts = nullptr, *h_counts = nullptr;
		kwage_hit *d_all = nullptr, *h_all = nullptr;
		NODE_HIP(hipMalloc((void**)&d_counts, (size_t)n_ranks*sizeof(uint64_t)));
		NODE_HIP(hipHostMalloc((void**)&h_counts, (size_t)n_ranks*sizeof(uint64_t)));
		double sum_kernel_ms = 0, t_exchange = 0, t_file = 0;
		uint64_t n_batches = 0, n_records = 0;
		const double t_search0 = now_seconds();
		double t_first_begin = 0;

		// ---- the passes: every rank's budget to everyone, then every rank plans every rank's passes ---------------------------
		size_t n_passes = 1;
		vector<vector<Unit> > my_passes = node_plan_rank_passes("kwage_node", ctx, rank, n_ranks, groups, files, rehearsal, comm, stream,
		                                                        d_counts, h_counts, stats, &n_passes);
		double t_parse_wait = 0;

		{
		RankPipeline pipe(ctx, rank, cli.threshold, flags);

		// The gatherv of one finished step: counts to everyone (one ncclAllGather straight from the lists' counter words),
		// records in exact sizes to rank 0 (one grouped ncclSend / ncclRecv; RCCL has no gatherv); rank 0 files them.
		// The next step's searches are running on the device meanwhile.
		auto exchange_and_file = [&](Step *st) {
			const double t0 = now_seconds();
			const HitList &l = pipe.lists[st->list];
			const uint64_t n_mine = st->n;
			vector<uint64_t> counts((size_t)n_ranks);
			const kwage_hit *hits = nullptr;
			uint64_t total = 0;
			if(rehearsal){
				rehearse_gather(rehearsal, rank, n_ranks, l.d_hits, n_mine, counts, total);
				if(rank == 0 && total){
					if(total > host_cap){
						if(h_all){ (void)hipHostFree(h_all); }
						host_cap = total + total/4;
						NODE_HIP(hipHostMalloc((void**)&h_all, host_cap*sizeof(kwage_hit)));
					}
					memcpy(h_all, rehearsal->records(), total*sizeof(kwage_hit));
					hits = h_all;
				}
				pthread_barrier_wait(&rehearsal->barrier);            // (the segment is free for the next batch)
			}
			else{
				// (the step's searches have been collected: the counter word holds the list's final count)
				node_counts_start(l.d_count, d_counts, h_counts, n_ranks, comm, stream);
				pipe.wait_feeding(stream);
				for(int r = 0; r < n_ranks; ++r){ counts[(size_t)r] = h_counts[r]; total += h_counts[r]; }
				if(counts[(size_t)rank] != n_mine){ throw string("the list's counter word disagrees with the count the search returned"); }
				if(rank == 0 && total > all_cap){
					if(d_all){ (void)hipFree(d_all); }
					all_cap = total + total/4;
					NODE_HIP(hipMalloc((void**)&d_all, all_cap*sizeof(kwage_hit)));
				}
				if(rank == 0 && total > host_cap){
					if(h_all){ (void)hipHostFree(h_all); }
					host_cap = total + total/4;
					NODE_HIP(hipHostMalloc((void**)&h_all, host_cap*sizeof(kwage_hit)));
				}
				node_send_recv(rank, n_ranks, counts, l.d_hits, n_mine, d_all, comm, stream);
				if(rank == 0 && total){
					// rank 0's own records go to the host straight from its list, the other ranks' from the gathered block
					if(n_mine){ NODE_HIP(hipMemcpyAsync(h_all, l.d_hits, n_mine*sizeof(kwage_hit), hipMemcpyDeviceToHost, stream)); }
					if(total > n_mine){ NODE_HIP(hipMemcpyAsync(h_all + n_mine, d_all + n_mine, (total - n_mine)*sizeof(kwage_hit), hipMemcpyDeviceToHost, stream)); }
					hits = h_all;
				}
				pipe.wait_feeding(stream);      // (a sender's list is refilled two steps on: the send has left it)
			}
			const double t1 = now_seconds();
			t_exchange += t1 - t0;

			if(rank == 0 && total){
				kwage_sort_hits(h_all, total);                     // by (query, global column): groups, ranks and files in order
				const QueryBatch &q = st->q;
				// num_query_kmer depends on the k-mer length only; lengths of which this rank holds no group (it searched none
				// of them) are the one case that still needs a k-mer stage of its own
				for(const NodeGroup &g : groups){
					if(st->nk.count(g.params.kmer_len)){ continue; }
					while(!pipe.flying.empty()){ pipe.collect_oldest(); pipe.pump(); }      // (kwage_hash_batch wants the context's slots idle)
					vector<uint64_t> off(q.size() + 1);
					vector<uint32_t> nk(q.size());
					check(kwage_hash_batch(ctx, &g.params, st->b, off.data(), nk.data(), nullptr, nullptr));
					st->nk[g.params.kmer_len] = std::move(nk);
				}
				pipe.pump();
				Findings &found = *st->found;
				for(uint64_t i = 0; i < total; ){
					const uint32_t qi = hits[i].query;
					const size_t qid = q.ids[qi];
					vector<Match> &dst = found.by_query.try_emplace(found.by_query.end(), qid)->second;
					if(!q.deflines.empty()){ found.defline.try_emplace(found.defline.end(), qid, q.deflines[qi]); }
					for(; i < total && hits[i].query == qi; ++i){
						// the last block that starts at or before the column
						const ColumnBlock &blk = *(upper_bound(blocks.begin(), blocks.end(), (uint64_t)hits[i].column,
						                                       [](uint64_t col, const ColumnBlock &b) { return col < b.first_global_column; }) - 1);
						Match m;
						m.num_kmers_found = hits[i].num_match;
						m.num_query_kmer = st->nk[blk.kmer_len][qi];
						m.file_index = blk.file_index;
						m.column = (uint32_t)(hits[i].column - blk.first_global_column);
						dst.push_back(m);
					}
				}
			}
			t_file += now_seconds() - t1;
			sum_kernel_ms += st->kernel_ms;
			n_records += total;
			++n_batches;
		};

		// batches stream through: batch i+1 is parsed (on its own thread) and its searches queued BEFORE batch i is
		// finished; batch i is exchanged and filed only AFTER batch i+2 has been queued (three lists rotate)
		unique_ptr<Step> open_step, done_step;             // begun, not finished yet; finished, not exchanged yet
		auto hand_over = [&](unique_ptr<Step> &st) {
			exchange_and_file(st.get());
			kwage_batch_destroy(st->b);
			st.reset();
		};
		auto run_source = [&](QuerySource &source, Findings &found) {
			PrefetchedQueries ahead(source, max_batch_bases);
			for(;;){
				unique_ptr<Step> st(new Step());
				const double t_fill = now_seconds();
				const bool more = ahead.fill(st->q, max_batch_bases);
				t_parse_wait += now_seconds() - t_fill;        // (every rank parses the query files, on a thread of its own: what the searches waited for it)
				if(!more){ break; }
				st->found = &found;
				if(t_first_begin == 0){ t_first_begin = now_seconds(); }
				pipe.begin(st.get());
				if(done_step){ hand_over(done_step); }
				if(open_step){ pipe.finish(open_step.get()); done_step = std::move(open_step); }
				open_step = std::move(st);
				open_step->q.bases = string();                      // resident on the device now
			}
		};
		Findings from_command_line_, from_files_;
		double t_load = 0;
		for(size_t pass = 0; pass < n_passes; ++pass){
			// ---- this pass's matrices (none: the rank's files are done -- it still takes part in every exchange) ------------
			vector<Unit> &units = my_passes[pass];
			const double t_l0 = now_seconds();
			for(Unit &u : units){
				NodeGroup &g = groups[u.gi];
				check(kwage_group_create(ctx, &g.params, u.span_columns, &u.mine));
				vector<const char*> paths;
				for(uint32_t fi : u.files){ paths.push_back(files[fi].path.c_str()); }
				vector<uint64_t> first(paths.size());
				check(kwage_group_add_db_files(u.mine, paths.data(), (uint32_t)paths.size(), first.data(), nullptr));
				if(first != u.first_column){ throw "main: the loaded layout differs from the planned one"; }
				check(kwage_group_finalize(u.mine));
			}
			t_load += now_seconds() - t_l0;
			pipe.units = &units;
			// the query sources are read once per pass (results are additive: a query's matches of this pass join those of the others)
			{
				CommandLineQueries typed(cli.query_seqs);
				run_source(typed, from_command_line_);
			}
			if(!cli.query_files.empty()){
				FileQueries disk(cli.query_files);
				run_source(disk, from_files_);
			}
			if(done_step){ hand_over(done_step); }
			if(open_step){ pipe.finish(open_step.get()); hand_over(open_step); }
			for(Unit &u : units){ if(u.mine){ kwage_group_destroy(u.mine); u.mine = nullptr; } }
		}
		const double t_search = now_seconds() - t_search0;
		if(stats && rank == 0){
			const double t_pipe = t_first_begin ? now_seconds() - t_first_begin : 0;
			fprintf(stderr, "[kwage_node] %llu batches, %llu records: first batch queued -> last batch filed %.3f ms wall (with the first batch's parsing %.3f ms); "
			                "sum of gather-kernel time (rank 0) %.3f ms = %.1f %% of it; exchange %.3f ms, filing %.3f ms (both beside the next batch's searches)\n",
			        (unsigned long long)n_batches, (unsigned long long)n_records, t_pipe*1e3, t_search*1e3,
			        sum_kernel_ms, t_pipe > 0 ? 100.0*sum_kernel_ms/(t_pipe*1e3) : 0.0, t_exchange*1e3, t_file*1e3);
			fprintf(stderr, "[kwage_node] %zu pass(es), loading %.3f s; waited %.3f ms for this rank's own query parser (every rank parses the query files on a prefetch thread)\n",
			        n_passes, t_load, t_parse_wait*1e3);
		}

		// (pipe is destroyed before the context)
		if(comm){ NODE_NCCL(ncclCommDestroy(comm)); }
		(void)hipFree(d_counts); (void)hipHostFree(h_counts);
		if(d_all){ (void)hipFree(d_all); }
		if(h_all){ (void)hipHostFree(h_all); }
		(void)hipStreamDestroy(stream);

		if(rank == 0){
			// order and report exactly as kwage does (kwage_main.cpp; reference kwage.cpp:191-315)
			write_report(cli, out, infos, from_command_line_, from_files_);
			cerr << "Search complete in " << (time(nullptr) - started) << " sec" << endl;
		}
		}
		kwage_shutdown(ctx);
		return EXIT_SUCCESS;
	});
}

}  // namespace

int main(int argc, char *argv[])
{
	setenv("GPU_MAX_HW_QUEUES", "8", 0);
	setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);          // dmabuf IPC (what RCCL needs on this host driver)
	setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);           // stdout is the report: RCCL's debug lines (NCCL_DEBUG) go to stderr
	Cli cli;
	vector<string> db_paths;
	const int status = guarded([&]() { return read_command_line(KWAGE_CLI, argc, argv, cli, db_paths); });
	if(status >= 0){ return status; }
	return node_main("kwage_node", db_paths, [&](int rank, int n_ranks, Bootstrap *boot, Rehearsal *rehearsal) {
		return run_rank(rank, n_ranks, boot, cli, db_paths, rehearsal);
	});
}
