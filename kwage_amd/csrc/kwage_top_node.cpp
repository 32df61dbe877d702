// kwage_amd/csrc/kwage_top_node.cpp -- `kwage_top_node`: kwage_top's command line on every GPU of a node, one process
// per GPU.  The options, the report and its bytes are kwage_top's (top_common.hpp, cli_common.hpp); the node machinery
// is kwage_node's (node_common.hpp): the sample axis sharded by whole files, global column numbers, passes when the
// database does not fit, one exchange per query batch over RCCL, the rehearsal on one device.
//
// Top k decomposes exactly: every shard uses the same floor f = kwage_query_threshold(t, n) (n counts the query's k-mers,
// not the shard's), so a query's global top k is the top k of the union of every shard's top k under one total order
// (score descending, file order, column ascending).  Per query batch and pass:
//   - every rank appends the top-k list of each of its units to one device list (kwage_search_topk_device_append, global
//     column numbers); a rank with more than one unit merges its list down to <= k per query (kwage_topk_merge_device);
//   - the lists go to rank 0 by kwage_node's exchange (count all-gather, grouped send / recv; under KWAGE_NODE_REHEARSE
//     through the shared host segment, uploaded again by rank 0);
//   - rank 0 merges the R lists on the device, copies back <= k records per query, maps each global column to (file,
//     column in file) and folds them into the query's running top k across passes (on the host: <= k per query).
// Every merge breaks ties by a table order[global column] that numbers the columns in file order, then column: global
// numbers are group-major, and a tie between groups must go to the earlier file, as in kwage_top.
//
//   KWAGE_NODE_STATS    1: also rank 0's device merges (launches, sources, records merged per exchange) on stderr
//   KWAGE_NODE_RANKS, KWAGE_NODE_PLAN, KWAGE_NODE_REHEARSE, KWAGE_NODE_COMM_TIMEOUT_S, KWAGE_BATCH_BASES,
//   KWAGE_MAX_GROUP_BYTES   as for kwage_node
#include "node_common.hpp"
#include "top_common.hpp"

namespace {

// a device block of hit records that grows on demand (its contents are not kept)
struct DevHits {
	kwage_hit *p = nullptr;
	uint64_t cap = 0;
	void need(uint64_t n)
	{
		if(n <= cap){ return; }
		if(p){ (void)hipFree(p); p = nullptr; cap = 0; }
		const uint64_t want = max<uint64_t>(n + n/4, 1024);
		NODE_HIP(hipMalloc((void**)&p, want*sizeof(kwage_hit)));
		cap = want;
	}
	~DevHits() { if(p){ (void)hipFree(p); } }
};

struct DevU32 {
	uint32_t *p = nullptr;
	uint64_t cap = 0;
	void need(uint64_t n)
	{
		if(n <= cap){ return; }
		if(p){ (void)hipFree(p); p = nullptr; cap = 0; }
		NODE_HIP(hipMalloc((void**)&p, n*sizeof(uint32_t)));
		cap = n;
	}
	~DevU32() { if(p){ (void)hipFree(p); } }
};

int run_rank(int rank, int n_ranks, Bootstrap *boot, const Cli &cli, const vector<string> &db_paths, Rehearsal *rehearsal)
{
	return guarded([&]() -> int {
		const time_t started = time(nullptr);
		const uint32_t k = cli.k;
		ofstream fout;
		if(rank == 0 && !open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;

		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, rank == 0 ? &infos : nullptr, rank == 0);
		vector<NodeGroup> groups = plan_groups(files, n_ranks);
		vector<ColumnBlock> blocks;          // ascending global columns (groups, ranks and files are numbered in order)
		uint64_t n_global = 0;
		for(const NodeGroup &g : groups){
			for(size_t r = 0; r < (size_t)n_ranks; ++r){
				for(size_t f = 0; f < g.share[r].files.size(); ++f){
					blocks.push_back(ColumnBlock{g.base[r] + g.share[r].first_column[f], g.share[r].files[f], g.params.kmer_len});
				}
				n_global = max(n_global, g.base[r] + g.share[r].span_columns);
			}
		}
		// the tie order: the real columns numbered file after file, column after column; the pad columns between file blocks
		// (never reported) after them, so that the table is injective
		vector<uint32_t> order(max<uint64_t>(n_global, 1), 0);
		{
			vector<uint64_t> first_of(files.size(), 0);
			for(const ColumnBlock &b : blocks){ first_of[b.file_index] = b.first_global_column; }
			vector<char> real(order.size(), 0);
			uint64_t next = 0;
			for(size_t fi = 0; fi < files.size(); ++fi){
				for(uint64_t c = 0; c < files[fi].header.num_filter; ++c){ order[first_of[fi] + c] = (uint32_t)next++; real[first_of[fi] + c] = 1; }
			}
			for(size_t i = 0; i < order.size(); ++i){ if(!real[i]){ order[i] = (uint32_t)next++; } }
		}

		kwage_ctx *ctx = nullptr;
		check(kwage_init(rehearsal ? 0 : rank, &ctx));
		one_shot_placement(ctx);
		ncclComm_t comm = nullptr;
		hipStream_t stream;
		NODE_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		if(!rehearsal){ comm = node_comm_init(rank, n_ranks, boot); }

		const uint64_t max_batch_bases = env_u64("KWAGE_BATCH_BASES", 64ull << 20);
		const bool stats = env_u64("KWAGE_NODE_STATS", 0) != 0;
		uint64_t *d_counts = nullptr, *h_counts = nullptr, *d_count = nullptr;
		uint32_t *d_order = nullptr;
		NODE_HIP(hipMalloc((void**)&d_counts, (size_t)n_ranks*sizeof(uint64_t)));
		NODE_HIP(hipHostMalloc((void**)&h_counts, (size_t)n_ranks*sizeof(uint64_t)));
		NODE_HIP(hipMalloc((void**)&d_count, sizeof(uint64_t)));
		NODE_HIP(hipMalloc((void**)&d_order, order.size()*sizeof(uint32_t)));
		NODE_HIP(hipMemcpy(d_order, order.data(), order.size()*sizeof(uint32_t), hipMemcpyHostToDevice));
		size_t n_passes = 1;
		vector<vector<Unit> > my_passes = node_plan_rank_passes("kwage_top_node", ctx, rank, n_ranks, groups, files, rehearsal, comm, stream,
		                                                        d_counts, h_counts, stats, &n_passes);
		uint64_t n_batches = 0, n_exchange_merges = 0, n_local_merges = 0, exchange_records = 0, local_records = 0;
		Findings from_command_line, from_files;
		{
		DevHits appended, mine, gathered, merged;
		DevU32 nk_dev;
		vector<kwage_hit> h_merged;

		// one query batch against this pass's units, the exchange, and on rank 0 the merge and the fold
		auto run_batch = [&](const QueryBatch &q, vector<Unit> &units, Findings &found) {
			const uint32_t nq = (uint32_t)q.size();
			kwage_batch *b = nullptr;
			check(kwage_batch_create(ctx, q.bases.data(), q.offsets.data(), nq, &b));
			try{
				// ---- this rank's list: every unit's top k (global columns), merged down to <= k per query when there are several
				uint64_t n_mine = 0;
				const kwage_hit *d_mine = nullptr;
				// rank 0: num_query_kmer per k-mer length (it depends on nothing else), taken from its own searches
				map<uint32_t, vector<uint32_t> > nk;
				if(units.empty()){ NODE_HIP(hipMemset(d_count, 0, sizeof(uint64_t))); }
				else{
					appended.need((uint64_t)units.size()*nq*k);
					for(size_t ui = 0; ui < units.size(); ++ui){
						const bool want_nk = rank == 0 && nq && !nk.count(units[ui].kmer_len);
						if(want_nk){ nk_dev.need(nq); }
						check(kwage_search_topk_device_append(units[ui].mine, b, k, cli.threshold, 0, appended.p, appended.cap, d_count,
						                                      (uint32_t)units[ui].base, ui == 0 ? 1 : 0, want_nk ? nk_dev.p : nullptr, &n_mine));
						if(want_nk){
							vector<uint32_t> &v = nk[units[ui].kmer_len];
							v.resize(nq);
							NODE_HIP(hipMemcpy(v.data(), nk_dev.p, (size_t)nq*sizeof(uint32_t), hipMemcpyDeviceToHost));
						}
					}
					d_mine = appended.p;
					if(units.size() > 1){
						mine.need((uint64_t)nq*k);
						check(kwage_topk_merge_device(ctx, appended.p, n_mine, nq, k, d_order, order.size(), mine.p, mine.cap, d_count));
						NODE_HIP(hipMemcpy(&n_mine, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost));
						d_mine = mine.p;
						++n_local_merges;
						local_records += n_mine;
					}
				}
				// ---- the exchange: every rank's list to rank 0, rank 0's own first --------------------------------------------
				vector<uint64_t> counts((size_t)n_ranks);
				uint64_t total = 0;
				if(rehearsal){
					rehearse_gather(rehearsal, rank, n_ranks, d_mine, n_mine, counts, total);
					if(rank == 0 && total){
						gathered.need(total);
						NODE_HIP(hipMemcpy(gathered.p, rehearsal->records(), total*sizeof(kwage_hit), hipMemcpyHostToDevice));
					}
					pthread_barrier_wait(&rehearsal->barrier);            // (the segment is free for the next batch)
				}
				else{
					node_counts_start(d_count, d_counts, h_counts, n_ranks, comm, stream);
					NODE_HIP(hipStreamSynchronize(stream));
					for(int r = 0; r < n_ranks; ++r){ counts[(size_t)r] = h_counts[r]; total += h_counts[r]; }
					if(counts[(size_t)rank] != n_mine){ throw string("the list's counter word disagrees with the count the search returned"); }
					if(rank == 0){ gathered.need(total); }
					node_send_recv(rank, n_ranks, counts, d_mine, n_mine, gathered.p, comm, stream);
					if(rank == 0 && n_mine){ NODE_HIP(hipMemcpyAsync(gathered.p, d_mine, n_mine*sizeof(kwage_hit), hipMemcpyDeviceToDevice, stream)); }
					NODE_HIP(hipStreamSynchronize(stream));
				}
				++n_batches;
				// ---- rank 0: the R lists merged on the device, <= k records per query back, folded into the running top k -----
				if(rank == 0 && total){
					merged.need((uint64_t)nq*k);
					check(kwage_topk_merge_device(ctx, gathered.p, total, nq, k, d_order, order.size(), merged.p, merged.cap, d_count));
					++n_exchange_merges;
					exchange_records += total;
					uint64_t n_out = 0;
					NODE_HIP(hipMemcpy(&n_out, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost));
					h_merged.resize(n_out);
					if(n_out){ NODE_HIP(hipMemcpy(h_merged.data(), merged.p, n_out*sizeof(kwage_hit), hipMemcpyDeviceToHost)); }
					for(uint64_t i = 0; i < n_out; ){
						const uint32_t qi = h_merged[i].query;
						const size_t id = q.ids[qi];
						vector<Match> &best = found.by_query[id];
						for(; i < n_out && h_merged[i].query == qi; ++i){
							const ColumnBlock &blk = *(upper_bound(blocks.begin(), blocks.end(), (uint64_t)h_merged[i].column,
							                                       [](uint64_t col, const ColumnBlock &bl) { return col < bl.first_global_column; }) - 1);
							if(!nk.count(blk.kmer_len)){      // a k-mer length of which rank 0 holds no unit in this pass: a k-mer stage, once
								const NodeGroup &g = *find_if(groups.begin(), groups.end(), [&](const NodeGroup &x) { return x.params.kmer_len == blk.kmer_len; });
								vector<uint64_t> off((size_t)nq + 1);
								vector<uint32_t> &v = nk[blk.kmer_len];
								v.resize(nq);
								check(kwage_hash_batch(ctx, &g.params, b, off.data(), v.data(), nullptr, nullptr));
							}
							best.push_back(Match{h_merged[i].num_match, nk[blk.kmer_len][qi], blk.file_index,
							                     (uint32_t)(h_merged[i].column - blk.first_global_column)});
						}
						if(best.size() > k){
							partial_sort(best.begin(), best.begin() + k, best.end(), better);
							best.resize(k);
						}
						if(!q.deflines.empty()){ found.defline.emplace(id, q.deflines[qi]); }
					}
				}
			}
			catch(...){ kwage_batch_destroy(b); throw; }
			kwage_batch_destroy(b);
		};

		for(size_t pass = 0; pass < n_passes; ++pass){
			vector<Unit> &units = my_passes[pass];
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
			// the query sources are read once per pass; every rank reads them and makes the same batches
			CommandLineQueries typed(cli.query_seqs);
			FileQueries from_disk(cli.query_files);
			for(QuerySource *src : {(QuerySource*)&typed, (QuerySource*)&from_disk}){
				for(;;){
					QueryBatch q;
					if(!src->fill(q, max_batch_bases)){ break; }
					run_batch(q, units, (src == &typed) ? from_command_line : from_files);
				}
			}
			for(Unit &u : units){ if(u.mine){ kwage_group_destroy(u.mine); u.mine = nullptr; } }
		}
		}
		if(stats){
			// (one write per rank: the ranks share stderr)
			if(rank == 0){
				fprintf(stderr, "[kwage_top_node] rank 0: %llu batches, %zu pass(es); exchange merges %llu of %d sources, %llu records merged (%.1f per exchange); "
				                "local merges %llu, %llu records out\n",
				        (unsigned long long)n_batches, n_passes, (unsigned long long)n_exchange_merges, n_ranks, (unsigned long long)exchange_records,
				        n_exchange_merges ? (double)exchange_records/n_exchange_merges : 0.0, (unsigned long long)n_local_merges, (unsigned long long)local_records);
			}
			else{
				fprintf(stderr, "[kwage_top_node] rank %d: local merges %llu, %llu records out\n", rank, (unsigned long long)n_local_merges,
				        (unsigned long long)local_records);
			}
		}
		if(comm){ NODE_NCCL(ncclCommDestroy(comm)); }
		(void)hipFree(d_counts); (void)hipHostFree(h_counts); (void)hipFree(d_count); (void)hipFree(d_order);
		(void)hipStreamDestroy(stream);
		kwage_shutdown(ctx);

		if(rank == 0){
			// each query's rows in the order `kwage` prints them, written as kwage_top writes them
			write_report(cli, out, infos, from_command_line, from_files);
			cerr << "Search complete in " << (time(nullptr) - started) << " sec" << endl;
		}
		return EXIT_SUCCESS;
	});
}

}  // namespace

int main(int argc, char *argv[])
{
	setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);          // dmabuf IPC (what RCCL needs on this host driver)
	setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);           // stdout is the report: RCCL's debug lines (NCCL_DEBUG) go to stderr
	Cli cli;
	vector<string> db_paths;
	const int status = guarded([&]() { return read_command_line(TOP_CLI, argc, argv, cli, db_paths); });
	if(status >= 0){ return status; }
	return node_main("kwage_top_node", db_paths, [&](int rank, int n_ranks, Bootstrap *boot, Rehearsal *rehearsal) {
		return run_rank(rank, n_ranks, boot, cli, db_paths, rehearsal);
	});
}
