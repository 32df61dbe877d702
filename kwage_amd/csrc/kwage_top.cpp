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
#include "cli_common.hpp"

namespace {

const char *const TOP_USAGE_LINES[] = {
	"Usage for kwage_top (the k best-scoring samples per query):",
	"\t-k <number of samples per query> (1 to 1024)",
	"\t[-o <output file>] (default is stdout)",
	"\t[--o.csv (output CSV) | --o.json (output JSON)]",
	"\t[-t <search threshold>] (default is 0: the k best, whatever their score)",
	"\t-d <database search path> (can be repeated)",
	"\t[-i <input sequence file>] (can be repeated)",
	"\t[<DNA sequence>] (can be repeated)",
};
static_assert(KWAGE_TOPK_MAX == 1024u, "TOP_USAGE_LINES quotes the cap");

// -k's value: decimal digits only, 1 .. KWAGE_TOPK_MAX.  Returns the complaint, or an empty string.
string parse_k(const char *text, uint32_t &k)
{
	if(!text){ return "Please provide the number of samples per query (-k)"; }
	const string s(text);
	const bool digits = !s.empty() && s.size() <= 9 && all_of(s.begin(), s.end(), [](char c) { return c >= '0' && c <= '9'; });
	const unsigned long v = digits ? strtoul(s.c_str(), nullptr, 10) : 0;
	if(!digits || v < 1 || v > KWAGE_TOPK_MAX){
		return "Please provide: 1 <= -k <= " + to_string(KWAGE_TOPK_MAX) + " (got \"" + s + "\")";
	}
	k = (uint32_t)v;
	return string();
}

// kwage's flags (FLAG_TABLE) plus -k.  Every complaint is reported before a device is touched; returns the exit status
// to end with, or -1 to go on.
int read_top_command_line(int argc, char *argv[], Cli &cli, uint32_t &k, vector<string> &db_files)
{
	string shorts = "k:";
	vector<struct option> longs;
	for(const FlagSpec &f : FLAG_TABLE){
		if(f.long_name){ longs.push_back({f.long_name, f.takes_value ? required_argument : no_argument, nullptr, f.code}); }
		else{ shorts += (char)f.code; if(f.takes_value){ shorts += ':'; } }
	}
	longs.push_back({nullptr, 0, nullptr, 0});
	opterr = 0;
	cli.threshold = 0.0f;
	cli.show_usage = (argc == 1);
	const char *k_text = nullptr;
	for(int code; (code = getopt_long(argc, argv, shorts.c_str(), longs.data(), nullptr)) != -1; ){
		if(code == 'k'){ k_text = optarg; continue; }
		if(code == '?' && optopt == 'k'){ k_text = ""; continue; }       // -k without its value
		const FlagSpec *f = find_if(begin(FLAG_TABLE), end(FLAG_TABLE), [&](const FlagSpec &x) { return x.code == code; });
		if(f != end(FLAG_TABLE)){ f->apply(cli, optarg); }
	}
	if(cli.show_usage){
		for(const char *line : TOP_USAGE_LINES){ cerr << line << endl; }
		return argc == 1 ? EXIT_FAILURE : EXIT_SUCCESS;
	}
	const string k_err = parse_k(k_text, k);
	if(!k_err.empty()){ cerr << k_err << endl; return EXIT_FAILURE; }
	if(!(cli.threshold >= 0.0f && cli.threshold <= 1.0f)){ cerr << "Please provide: 0.0 <= search threshold <= 1.0" << endl; return EXIT_FAILURE; }
	cli.query_seqs.assign(argv + optind, argv + argc);
	const string *bad_name = nullptr;
	for(const string &q : cli.query_files){ if(!bad_name && !accepted_query_name(q)){ bad_name = &q; } }
	if(bad_name){ cerr << "The query sequence file name, " << *bad_name << ", does not have an allowed file extension" << endl; return EXIT_FAILURE; }
	if(cli.query_files.empty() && cli.query_seqs.empty()){ cerr << "Please provide at least one query sequence or file" << endl; return EXIT_FAILURE; }
	find_database_files(cli.db_roots, db_files);
	if(db_files.empty()){ cerr << "Please provide at least one database file to search (-d)" << endl; return EXIT_FAILURE; }
	return -1;
}

// (score descending, file order, column ascending): the order in which a query's best samples are chosen
bool better(const Match &a, const Match &b)
{
	if(a.num_kmers_found != b.num_kmers_found){ return a.num_kmers_found > b.num_kmers_found; }
	return (a.file_index != b.file_index) ? (a.file_index < b.file_index) : (a.column < b.column);
}

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
