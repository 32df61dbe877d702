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
// Environment: KWAGE_DEVICE (HIP device index, default 0), KWAGE_BATCH_BASES (bases per query batch, default 64 Mi).
#include "top_common.hpp"

namespace {

// A batch of queries on the device and where its results go.
struct ResidentBatch {
	QueryBatch q;
	kwage_batch *b = nullptr;
	Findings *to = nullptr;
};

}  // namespace

int main(int argc, char *argv[])
{
	try{
		const time_t started = time(nullptr);
		Cli cli;
		uint32_t k = 0;
		vector<string> db_paths;
		const int status = read_top_command_line(argc, argv, cli, k, db_paths);
		if(status >= 0){ return status; }

		ofstream fout;
		if(!cli.output_path.empty()){
			fout.open(cli.output_path.c_str());
			if(!fout){
				cerr << "Unable to open " << cli.output_path << " for writing" << endl;
				return EXIT_FAILURE;
			}
		}
		ostream &out = fout.is_open() ? fout : cout;

		vector<DbFileEntry> files(db_paths.size());
		vector<DbInfo> infos(db_paths.size());
		for(size_t i = 0; i < db_paths.size(); ++i){
			files[i].path = db_paths[i];
			if(kwage_db_read_header(files[i].path.c_str(), &files[i].header) != KWAGE_OK){
				cerr << kwage_last_error() << endl;
				throw "main: I/O error";
			}
			string err;
			if(!infos[i].open(files[i].path, err)){
				cerr << err << endl;
				throw "main: Unable to read header";
			}
		}

		// ---- every query, in batches (the query set stays in host and device memory for the whole run) ------------------
		const uint64_t max_bases = env_u64("KWAGE_BATCH_BASES", 64ull << 20);
		Findings from_command_line, from_files;
		deque<ResidentBatch> batches;
		{
			CommandLineQueries typed(cli.query_seqs);
			FileQueries from_disk(cli.query_files);
			for(QuerySource *src : {(QuerySource*)&typed, (QuerySource*)&from_disk}){
				for(;;){
					ResidentBatch rb;
					if(!src->fill(rb.q, max_bases)){ break; }
					rb.to = (src == &typed) ? &from_command_line : &from_files;
					batches.push_back(std::move(rb));
				}
			}
		}

		kwage_ctx *ctx = nullptr;
		check(kwage_init((int)env_u64("KWAGE_DEVICE", 0), &ctx));
		one_shot_placement(ctx);
		try{
			for(ResidentBatch &rb : batches){
				check(kwage_batch_create(ctx, rb.q.bases.data(), rb.q.offsets.data(), (uint32_t)rb.q.size(), &rb.b));
			}
			// ---- file by file: search, then fold into each query's running top k -----------------------------------------
			for(size_t fi = 0; fi < files.size(); ++fi){
				const kwage_db_header &h = files[fi].header;
				kwage_params p{h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func};
				kwage_group *g = nullptr;
				check(kwage_group_create(ctx, &p, h.num_filter, &g));
				try{
					uint64_t first = 0;
					uint32_t nf = 0;
					check(kwage_group_add_db_file(g, files[fi].path.c_str(), &first, &nf));
					check(kwage_group_finalize(g));
					for(ResidentBatch &rb : batches){
						kwage_result *r = nullptr;
						check(kwage_search_topk(g, rb.b, k, cli.threshold, 0, &r));
						for(uint64_t i = 0; i < r->n_hits; ){
							const uint32_t q = r->hits[i].query;
							const size_t id = rb.q.ids[q];
							vector<Match> &best = rb.to->by_query[id];
							for(; i < r->n_hits && r->hits[i].query == q; ++i){
								best.push_back(Match{r->hits[i].num_match, r->num_query_kmer[q], (uint32_t)fi, (uint32_t)(r->hits[i].column - first)});
							}
							if(best.size() > k){
								partial_sort(best.begin(), best.begin() + k, best.end(), better);
								best.resize(k);
							}
							if(!rb.q.deflines.empty()){ rb.to->defline.emplace(id, rb.q.deflines[q]); }
						}
						kwage_result_free(r);
					}
				}
				catch(...){ kwage_group_destroy(g); throw; }
				kwage_group_destroy(g);
			}
		}
		catch(...){
			for(ResidentBatch &rb : batches){ if(rb.b){ kwage_batch_destroy(rb.b); } }
			kwage_shutdown(ctx);
			throw;
		}
		for(ResidentBatch &rb : batches){ kwage_batch_destroy(rb.b); }
		kwage_shutdown(ctx);

		// ---- each query's rows in the order `kwage` prints them (kwage_main.cpp: file order and column, then hits) ---------
		for(Findings *f : {&from_command_line, &from_files}){
			for(auto &kv : f->by_query){
				sort(kv.second.begin(), kv.second.end(), [](const Match &a, const Match &b) {
					return (a.file_index != b.file_index) ? (a.file_index < b.file_index) : (a.column < b.column);
				});
				sort(kv.second.begin(), kv.second.end(), [](const Match &a, const Match &b) { return a.num_kmers_found > b.num_kmers_found; });
			}
		}
		unique_ptr<Report> report;
		if(cli.format == Cli::CSV){ report.reset(new CsvReport(out, infos)); }
		else{ report.reset(new JsonReport(out, cli.threshold, infos)); }
		report->begin(from_command_line.by_query.size() + from_files.by_query.size());
		for(const auto &kv : from_command_line.by_query){ report->query("command line seq " + to_string(kv.first), kv.second); }
		for(const auto &kv : from_files.by_query){ report->query(from_files.defline[kv.first], kv.second); }
		report->end();
		cerr << "Search complete in " << (time(nullptr) - started) << " sec" << endl;
	}
	catch(const char *error){
		cerr << "Caught the error " << error << endl;
		return EXIT_FAILURE;
	}
	catch(const string &error){
		cerr << "Caught the error " << error << endl;
		return EXIT_FAILURE;
	}
	catch(...){
		cerr << "Caught an unhandled error" << endl;
		return EXIT_FAILURE;
	}
	return EXIT_SUCCESS;
}
