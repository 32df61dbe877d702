// kwage_amd/csrc/kwage_presence.cpp -- the `kwage_presence` command-line program: for every query, which samples of the
// database hold it at the threshold, as one tab-separated 0 / 1 matrix (kwage_search_presence).  No counterpart in the
// reference.  The options are kwage's (cli_common.hpp: -d, -i, positional sequences, -o, -t with kwage's default of 1);
// there is no report format.
//
//   query <TAB> num_kmers <TAB> passing <TAB> <run accession of sample 0> <TAB> <run accession of sample 1> ...
//   <query name> <TAB> <distinct k-mers> <TAB> <samples that pass> <TAB> <0 | 1 for sample 0> <TAB> ...
//
// A cell is 1 exactly where `kwage -t <threshold>` reports the (query, sample) pair.  Samples come in database order
// (files as found, columns within a file); queries in kwage's order: the sequences of the command line ("command line
// seq <i>") first, then the records of the -i files under their deflines.  Every query has a line, also one without
// k-mers (all zeros).  The database is searched file by file, one group per file, like kwage_scores: it never has to
// fit the device at once.  The matrix does have to fit the host: every query's row of samples / 8 bytes (and every
// query batch on the device) stays resident until all files are searched, then it is printed; the usage text says so.
//
// Environment: KWAGE_DEVICE (HIP device index, default 0), KWAGE_BATCH_BASES (bases per query batch, default 64 Mi).
#include "cli_common.hpp"

namespace {

const char *const PRESENCE_USAGE_LINES[] = {
	"Usage for kwage_presence (which samples hold each query: a tab-separated 0/1 matrix):",
	"\t[-o <output file>] (default is stdout)",
	"\t[-t <search threshold>] (default is 1)",
	"\t-d <database search path> (can be repeated)",
	"\t[-i <input sequence file>] (can be repeated)",
	"\t[<DNA sequence>] (can be repeated)",
	"\t(the whole matrix, samples / 8 bytes per query, is held in host memory until it is printed)",
};

// kwage's -o, -t, -d, -i and -h out of FLAG_TABLE; anything else (-k, the report formats) shows the usage text.  Every
// complaint is reported before a device is touched; returns the exit status to end with, or -1 to go on.
int read_presence_command_line(int argc, char *argv[], Cli &cli, vector<string> &db_files)
{
	string shorts;
	for(const FlagSpec &f : FLAG_TABLE){
		if(f.long_name){ continue; }
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
		for(const char *line : PRESENCE_USAGE_LINES){ cerr << line << endl; }
		return (argc == 1 || refused) ? EXIT_FAILURE : EXIT_SUCCESS;
	}
	cli.query_seqs.assign(argv + optind, argv + argc);
	if(!(cli.threshold > 0.0f && cli.threshold <= 1.0f)){ cerr << "Please provide: 0.0 < search threshold <= 1.0" << endl; return EXIT_FAILURE; }
	const string *bad_name = nullptr;
	for(const string &q : cli.query_files){ if(!bad_name && !accepted_query_name(q)){ bad_name = &q; } }
	if(bad_name){ cerr << "The query sequence file name, " << *bad_name << ", does not have an allowed file extension" << endl; return EXIT_FAILURE; }
	if(cli.query_files.empty() && cli.query_seqs.empty()){ cerr << "Please provide at least one query sequence or file" << endl; return EXIT_FAILURE; }
	find_database_files(cli.db_roots, db_files);
	if(db_files.empty()){ cerr << "Please provide at least one database file to search (-d)" << endl; return EXIT_FAILURE; }
	return -1;
}

// A batch of queries on the device, and its block of the matrix: one row of row_bytes per query, bit s = sample s.
struct ResidentBatch {
	QueryBatch q;
	kwage_batch *b = nullptr;
	bool typed = false;                 // from the command line
	vector<uint32_t> nkmer;             // per query, for the k-mer length of the database's first file
	vector<uint32_t> passing;           // per query, summed over the files
	vector<uint8_t> bits;               // [query][row_bytes]
};

}  // namespace

int main(int argc, char *argv[])
{
	try{
		Cli cli;
		vector<string> db_paths;
		const int status = read_presence_command_line(argc, argv, cli, db_paths);
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
		const uint64_t row_bytes = (samples + 7)/8;

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
					rb.passing.assign(rb.q.size(), 0);
					try{ rb.bits.assign(rb.q.size()*row_bytes, 0); }
					catch(const std::bad_alloc&){
						cerr << "The matrix does not fit in host memory: " << samples << " samples / 8 bytes for every query" << endl;
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
			// ---- file by file: the file's bitmap, its real columns copied to their place in each batch's block ---------------
			vector<uint8_t> part;
			vector<uint32_t> passing;
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
					const uint64_t w = (kwage_group_row_bytes(g) + 15)/16*16;
					for(ResidentBatch &rb : batches){
						part.resize(std::max<uint64_t>(rb.q.size()*w, 1));
						passing.assign(std::max<size_t>(rb.q.size(), 1), 0);
						check(kwage_search_presence(g, rb.b, cli.threshold, part.data(), w, passing.data(), fi == 0 ? rb.nkmer.data() : nullptr, KWAGE_SEARCH_EARLY_EXIT, nullptr));
						for(size_t q = 0; q < rb.q.size(); ++q){
							rb.passing[q] += passing[q];
							if(!passing[q]){ continue; }
							const uint8_t *src = part.data() + q*w;
							uint8_t *dst = rb.bits.data() + q*row_bytes;
							for(uint64_t c = 0; c < nf; ++c){
								const uint64_t from = first + c, to = files[fi].first_column + c;
								if((src[from >> 3] >> (from & 7)) & 1u){ dst[to >> 3] |= (uint8_t)(1u << (to & 7)); }
							}
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
		to.put("query\tnum_kmers\tpassing");
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
				to.put('\t'); to.put((uint64_t)rb.passing[q]);
				const uint8_t *row = rb.bits.data() + q*row_bytes;
				for(uint64_t c = 0; c < samples; ++c){ to.put('\t'); to.put((row[c >> 3] >> (c & 7)) & 1u ? '1' : '0'); to.drain(); }
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
