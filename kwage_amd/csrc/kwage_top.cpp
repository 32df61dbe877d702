// kwage_amd/csrc/kwage_top.cpp -- the `kwage_top` command-line program: for each query, the k samples of the database
// with the most k-mer matches (kwage_search_topk).  No counterpart in the reference.  The options are kwage's
// (cli_common.hpp: -d, -i, positional sequences, -o, --o.csv / --o.json, -t) plus a required -k <n>; -t defaults to 0
// ("the k best, whatever their score") and may be anything in [0, 1].  The report is kwage's CSV / JSON, byte for byte
// the layout `kwage` writes: for t > 0 each query's rows are the first k rows `kwage -t t` prints for it (the same
// scores in the same order; the same samples unless a run of equal scores straddles row k).
//
// The database is searched file by file: one group per file, every query batch searched against it, and a running
// top k per query kept on the host -- top k merges associatively, so the database never has to fit the device at once.
// Ties are broken by (score descending, file order, column ascending).
//
// Environment: KWAGE_DEVICE, KWAGE_BATCH_BASES (file_search.hpp).
#include "file_search.hpp"
#include "top_common.hpp"

namespace {

struct Nothing {};          // a batch keeps nothing of its own: its results go to the Findings of its query source

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		const time_t started = time(nullptr);
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(TOP_CLI, argc, argv, cli, db_paths);
		if(status >= 0){ return status; }
		ofstream fout;
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;
		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, &infos);

		deque<ResidentBatch<Nothing> > batches;
		read_queries(cli, batches, [](ResidentBatch<Nothing> &) { return true; });
		// ---- file by file: search, then fold into each query's running top k ---------------------------------------------
		const uint32_t k = cli.k;
		Findings from_command_line, from_files;
		search_file_by_file(files, batches, [&](size_t fi, const FileGroup &g, ResidentBatch<Nothing> &rb) {
			Findings &to = rb.typed ? from_command_line : from_files;
			kwage_result *r = nullptr;
			check(kwage_search_topk(g.get(), rb.b, k, cli.threshold, 0, &r));
			for(uint64_t i = 0; i < r->n_hits; ){
				const uint32_t q = r->hits[i].query;
				const size_t id = rb.q.ids[q];
				vector<Match> &best = to.by_query[id];
				for(; i < r->n_hits && r->hits[i].query == q; ++i){
					best.push_back(Match{r->hits[i].num_match, r->num_query_kmer[q], (uint32_t)fi, (uint32_t)(r->hits[i].column - g.first)});
				}
				if(best.size() > k){
					partial_sort(best.begin(), best.begin() + k, best.end(), better);
					best.resize(k);
				}
				if(!rb.q.deflines.empty()){ to.defline.emplace(id, rb.q.deflines[q]); }
			}
			kwage_result_free(r);
		});

		// ---- each query's rows in the order `kwage` prints them (file order and column, then hits) --------------------------
		write_report(cli, out, infos, from_command_line, from_files);
		cerr << "Search complete in " << (time(nullptr) - started) << " sec" << endl;
		return EXIT_SUCCESS;
	});
}
