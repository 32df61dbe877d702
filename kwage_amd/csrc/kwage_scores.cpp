// kwage_amd/csrc/kwage_scores.cpp -- the `kwage_scores` command-line program: every query's k-mer match count for every
// sample of the database, as one tab-separated matrix (kwage_search_scores).  No counterpart in the reference.  The
// options are kwage's (cli_common.hpp: -d, -i, positional sequences, -o); there is no threshold and no report format.
//
//   query <TAB> num_kmers <TAB> <run accession of sample 0> <TAB> <run accession of sample 1> ...
//   <query name> <TAB> <distinct k-mers> <TAB> <matches in sample 0> <TAB> ...
//
// Samples come in database order (files as found, columns within a file); queries in kwage's order: the sequences of
// the command line ("command line seq <i>") first, then the records of the -i files under their deflines.  Every query
// has a line, also one without k-mers (all zeros).  The database is searched file by file, one group per file, like
// kwage_top: it never has to fit the device at once.  The matrix does have to fit the host: every query's row of
// samples x 4 bytes (and every query batch on the device) stays resident until all files are searched, then it is printed
// (400 MB per 1000 queries at 100 k samples); the usage text says so.
//
// Environment: KWAGE_DEVICE (HIP device index, default 0), KWAGE_BATCH_BASES (bases per query batch, default 64 Mi).
#include "cli_common.hpp"

namespace {

const char *const SCORES_USAGE_LINES[] = {
	"Usage for kwage_scores (every query's match count for every sample, tab-separated):",
	"\t[-o <output file>] (default is stdout)",
	"\t-d <database search path> (can be repeated)",
	"\t[-i <input sequence file>] (can be repeated)",
	"\t[<DNA sequence>] (can be repeated)",
	"\t(the whole matrix, queries x samples x 4 bytes, is held in host memory until it is printed)",
};

// kwage's -o, -d, -i and -h out of FLAG_TABLE; anything else (-t, -k, the report formats) shows the usage text.  Every
// complaint is reported before a device is touched; returns the exit status to end with, or -1 to go on.
int read_scores_command_line(int argc, char *argv[], Cli &cli, vector<string> &db_files)
{
	string shorts;
	for(const FlagSpec &f : FLAG_TABLE){
		if(f.long_name || f.code == 't'){ continue; }
		shorts += (char)f.code;
		if(f.takes_value){ shorts += ':'; }
	}
	const struct option longs[] = {{nullptr, 0, nullptr, 0}};
	opterr = 0;
	cli.show_usage = (argc == 1);
	bool refused = false;
	for(int code; (code = getopt_long(argc, argv, shorts.c_str(), longs, nullptr)) != -1; ){
		if(code == '?'){ refused = true; }
		const FlagSpec *f = find_if(begin(FLAG_TABLE), end(FLAG_TABLE), [&](const FlagSpec &x) { return x.code == code; });
		if(f != end(FLAG_TABLE)){ f->apply(cli, optarg); }
	}
	if(cli.show_usage){
		for(const char *line : SCORES_USAGE_LINES){ cerr << line << endl; }
		return (argc == 1 || refused) ? EXIT_FAILURE : EXIT_SUCCESS;
	}
	cli.query_seqs.assign(argv + optind, argv + argc);
	const string *bad_name = nullptr;
	for(const string &q : cli.query_files){ if(!bad_name && !accepted_query_name(q)){ bad_name = &q; } }
	if(bad_name){ cerr << "The query sequence file name, " << *bad_name << ", does not have an allowed file extension" << endl; return EXIT_FAILURE; }
	if(cli.query_files.empty() && cli.query_seqs.empty()){ cerr << "Please provide at least one query sequence or file" << endl; return EXIT_FAILURE; }
	find_database_files(cli.db_roots, db_files);
	if(db_files.empty()){ cerr << "Please provide at least one database file to search (-d)" << endl; return EXIT_FAILURE; }
	return -1;
}

// A batch of queries on the device, and its block of the matrix: one row per query, the files' real columns side by side.
struct ResidentBatch {
	QueryBatch q;
	kwage_batch *b = nullptr;
	bool typed = false;                 // from the command line
	vector<uint32_t> nkmer;             // per query, for the k-mer length of the database's first file
	vector<uint32_t> cells;             // [query][sample]
};

}  // namespace

int main(int argc, char *argv[])
{
	try{
		Cli cli;
		vector<string> db_paths;
		const int status = read_scores_command_line(argc, argv, cli, db_paths);
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
		uint64_t samples = 0;
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
			files[i].first_column = samples;            // (here: the file's first sample in the matrix)
			samples += files[i].header.num_filter;
		}

		// ---- every query, in batches (the query set stays in host and device memory for the whole run) ------------------
		const uint64_t max_bases = env_u64("KWAGE_BATCH_BASES", 64ull << 20);
		deque<ResidentBatch> batches;
		{
			CommandLineQueries typed(cli.query_seqs);
			FileQueries from_disk(cli.query_files);
			for(QuerySource *src : {(QuerySource*)&typed, (QuerySource*)&from_disk}){
				for(;;){
					ResidentBatch rb;
					if(!src->fill(rb.q, max_bases)){ break; }
					rb.typed = (src == &typed);
					rb.nkmer.assign(rb.q.size(), 0);
					try{ rb.cells.assign(rb.q.size()*samples, 0); }
					catch(const std::bad_alloc&){
						cerr << "The matrix does not fit in host memory: " << samples << " samples x 4 bytes for every query" << endl;
						return EXIT_FAILURE;
					}
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
			// ---- file by file: the file's matrix, its real columns copied to their place in each batch's block ---------------
			vector<uint32_t> part;
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
					const uint64_t span = kwage_group_column_span(g);
					for(ResidentBatch &rb : batches){
						part.resize(std::max<uint64_t>(rb.q.size()*span, 1));
						check(kwage_search_scores(g, rb.b, part.data(), span, fi == 0 ? rb.nkmer.data() : nullptr, 0, nullptr));
						for(size_t q = 0; q < rb.q.size(); ++q){
							memcpy(rb.cells.data() + q*samples + files[fi].first_column, part.data() + q*span + first, (size_t)nf*sizeof(uint32_t));
						}
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

		// ---- the matrix: header, then the queries in kwage's order (the batches were made in that order) -------------------
		TextSink to(out);
		to.put("query\tnum_kmers");
		for(size_t fi = 0; fi < files.size(); ++fi){
			for(uint32_t c = 0; c < files[fi].header.num_filter; ++c){
				FilterInfo info;
				if(!infos[fi].info(c, info)){ throw "binary_read<FilterInfo>: Unable to read FilterInfo"; }
				to.put('\t'); to.put(info.csv_string());
				to.drain();
			}
		}
		to.put('\n');
		for(const ResidentBatch &rb : batches){
			for(size_t q = 0; q < rb.q.size(); ++q){
				if(rb.typed){ to.put("command line seq "); to.put((uint64_t)rb.q.ids[q]); }
				else{ to.put(rb.q.deflines[q]); }
				to.put('\t'); to.put((uint64_t)rb.nkmer[q]);
				for(uint64_t c = 0; c < samples; ++c){ to.put('\t'); to.put((uint64_t)rb.cells[q*samples + c]); to.drain(); }
				to.put('\n');
			}
		}
		to.flush();
		out.flush();
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
