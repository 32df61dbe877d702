// kwage_amd/csrc/kwage_near.cpp -- the `kwage_near` command-line program: for samples of the database, named by run
// accession, the k samples whose Bloom filters are most like theirs, by Jaccard index of the set rows (the filter search,
// kwage_search_filter_scores).  No counterpart in the reference.  The options are kwage's -d and -o (cli_common.hpp),
// -k (top_common.hpp's parser; default 10) and the accessions, positional or with -s.
//
//   query <TAB> rank <TAB> sample <TAB> shared_bits <TAB> query_bits <TAB> sample_bits <TAB> jaccard
//
// jaccard = shared / (query_bits + sample_bits - shared) as a double (0 where that is empty), printed with %.6f; a query's
// lines come in the order (jaccard descending, file order, column ascending), ranks from 1.  The query sample itself is
// listed: it ranks first with 1.000000 unless an identical filter precedes it, which makes every run check itself.
//
// An accession is the first (file, column) carrying it, in database order; one found nowhere ends the program with a
// message that names it, before a device is opened.  Two passes, one group per file as in kwage_scores: the first loads
// only the files that hold a query sample and keeps their samples' row lists on the device (one filter set per such
// file), the second searches every file with every set.  Loading the few source files twice keeps the second pass one
// plain loop; a single pass would have to come back to the files searched before a later query sample's file was
// reached.  Files whose Bloom parameters differ from a query sample's are skipped for that sample: filters built
// differently are not comparable.
//
// Environment: KWAGE_DEVICE (HIP device index, default 0).
#include "top_common.hpp"

namespace {

const char *const NEAR_USAGE_LINES[] = {
	"Usage for kwage_near (the samples most like given samples of the database, by Jaccard index of their Bloom filters):",
	"\t[-k <number of samples per query sample>] (1 to 1024, default is 10)",
	"\t[-o <output file>] (default is stdout)",
	"\t-d <database search path> (can be repeated)",
	"\t[-s <run accession>] (can be repeated)",
	"\t[<run accession>] (can be repeated)",
};

// kwage's -o, -d and -h out of FLAG_TABLE, plus -k and -s; anything else shows the usage text.  Every complaint is
// reported before a device is touched; returns the exit status to end with, or -1 to go on.
int read_near_command_line(int argc, char *argv[], Cli &cli, uint32_t &k, vector<string> &accessions, vector<string> &db_files)
{
	const struct option longs[] = {{nullptr, 0, nullptr, 0}};
	opterr = 0;
	cli.show_usage = (argc == 1);
	bool refused = false;
	const char *k_text = "10";
	for(int code; (code = getopt_long(argc, argv, "k:s:o:d:h", longs, nullptr)) != -1; ){
		if(code == 'k'){ k_text = optarg; continue; }
		if(code == 's'){ accessions.push_back(optarg); continue; }
		if(code == '?' && optopt == 'k'){ k_text = ""; continue; }       // -k without its value
		if(code == '?'){ refused = true; }
		const FlagSpec *f = find_if(begin(FLAG_TABLE), end(FLAG_TABLE), [&](const FlagSpec &x) { return x.code == code; });
		if(f != end(FLAG_TABLE)){ f->apply(cli, optarg); }
	}
	if(cli.show_usage){
		for(const char *line : NEAR_USAGE_LINES){ cerr << line << endl; }
		return (argc == 1 || refused) ? EXIT_FAILURE : EXIT_SUCCESS;
	}
	const string k_err = parse_k(k_text, k);
	if(!k_err.empty()){ cerr << k_err << endl; return EXIT_FAILURE; }
	accessions.insert(accessions.end(), argv + optind, argv + argc);
	if(accessions.empty()){ cerr << "Please provide at least one run accession of a sample of the database" << endl; return EXIT_FAILURE; }
	find_database_files(cli.db_roots, db_files);
	if(db_files.empty()){ cerr << "Please provide at least one database file to search (-d)" << endl; return EXIT_FAILURE; }
	return -1;
}

struct Near {
	double jaccard;
	uint32_t file, column, shared, sample_bits;
};

// (jaccard descending, file order, column ascending)
bool nearer(const Near &a, const Near &b)
{
	if(a.jaccard != b.jaccard){ return a.jaccard > b.jaccard; }
	return (a.file != b.file) ? (a.file < b.file) : (a.column < b.column);
}

struct QuerySample {
	string accession;
	uint32_t file = 0, column = 0;      // where it lies
	uint32_t bits = 0;                  // its filter's set rows
	vector<Near> best;                  // the running top k
};

// The query samples of one source file, as one filter set on the device.
struct SourceSet {
	uint32_t file = 0;
	vector<uint32_t> queries;           // indices into the query samples, in the set's order
	kwage_filterset *fs = nullptr;
};

bool same_params(const kwage_db_header &a, const kwage_db_header &b)
{
	return a.kmer_len == b.kmer_len && a.num_hash == b.num_hash && a.log_2_filter_len == b.log_2_filter_len && a.hash_func == b.hash_func;
}

// One file as a finalized group of its own.
kwage_group *load_file(kwage_ctx *ctx, const DbFileEntry &f, uint64_t &first)
{
	const kwage_db_header &h = f.header;
	kwage_params p{h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func};
	kwage_group *g = nullptr;
	check(kwage_group_create(ctx, &p, h.num_filter, &g));
	try{
		uint32_t nf = 0;
		check(kwage_group_add_db_file(g, f.path.c_str(), &first, &nf));
		check(kwage_group_finalize(g));
	}
	catch(...){ kwage_group_destroy(g); throw; }
	return g;
}

}  // namespace

int main(int argc, char *argv[])
{
	try{
		Cli cli;
		uint32_t k = 10;
		vector<string> db_paths, accessions;
		const int status = read_near_command_line(argc, argv, cli, k, accessions, db_paths);
		if(status >= 0){ return status; }

		vector<DbFileEntry> files(db_paths.size());
		vector<DbInfo> infos(db_paths.size());
		vector<vector<string>> names(db_paths.size());          // run accession of every column
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
			names[i].resize(files[i].header.num_filter);
			for(uint32_t c = 0; c < files[i].header.num_filter; ++c){
				FilterInfo info;
				if(!infos[i].info(c, info)){ throw "binary_read<FilterInfo>: Unable to read FilterInfo"; }
				names[i][c] = info.csv_string();
			}
		}

		// ---- every accession to the first (file, column) that carries it --------------------------------------------------
		vector<QuerySample> queries(accessions.size());
		for(size_t q = 0; q < accessions.size(); ++q){
			queries[q].accession = accessions[q];
			bool found = false;
			for(size_t fi = 0; fi < files.size() && !found; ++fi){
				const auto at = find(names[fi].begin(), names[fi].end(), accessions[q]);
				if(at != names[fi].end()){
					queries[q].file = (uint32_t)fi;
					queries[q].column = (uint32_t)(at - names[fi].begin());
					found = true;
				}
			}
			if(!found){
				cerr << "No sample with the run accession " << accessions[q] << " in the database" << endl;
				return EXIT_FAILURE;
			}
		}
		vector<SourceSet> sets;
		for(size_t q = 0; q < queries.size(); ++q){
			auto at = find_if(sets.begin(), sets.end(), [&](const SourceSet &s) { return s.file == queries[q].file; });
			if(at == sets.end()){ sets.push_back(SourceSet()); at = sets.end() - 1; at->file = queries[q].file; }
			at->queries.push_back((uint32_t)q);
		}
		sort(sets.begin(), sets.end(), [](const SourceSet &a, const SourceSet &b) { return a.file < b.file; });

		ofstream fout;
		if(!cli.output_path.empty()){
			fout.open(cli.output_path.c_str());
			if(!fout){
				cerr << "Unable to open " << cli.output_path << " for writing" << endl;
				return EXIT_FAILURE;
			}
		}
		ostream &out = fout.is_open() ? fout : cout;

		kwage_ctx *ctx = nullptr;
		check(kwage_init((int)env_u64("KWAGE_DEVICE", 0), &ctx));
		one_shot_placement(ctx);
		try{
			// ---- first pass: the source files, their query samples' row lists kept on the device -----------------------------
			for(SourceSet &s : sets){
				uint64_t first = 0;
				kwage_group *g = load_file(ctx, files[s.file], first);
				try{
					vector<uint64_t> cols;
					for(uint32_t q : s.queries){ cols.push_back(first + queries[q].column); }
					check(kwage_filterset_from_columns(g, cols.data(), (uint32_t)cols.size(), &s.fs));
					vector<uint32_t> bits(cols.size());
					check(kwage_filterset_bit_counts(s.fs, bits.data()));
					for(size_t i = 0; i < cols.size(); ++i){ queries[s.queries[i]].bits = bits[i]; }
				}
				catch(...){ kwage_group_destroy(g); throw; }
				kwage_group_destroy(g);
			}
			// ---- second pass: every file against every set; each query sample's k best folded on the host ----------------------
			vector<uint32_t> part, column_bits;
			for(size_t fi = 0; fi < files.size(); ++fi){
				bool wanted = false;
				for(const SourceSet &s : sets){
					if(same_params(files[s.file].header, files[fi].header)){ wanted = true; continue; }
					for(uint32_t q : s.queries){
						cerr << "Skipping " << files[fi].path << " for " << queries[q].accession << ": its Bloom filter parameters differ from the sample's" << endl;
					}
				}
				if(!wanted){ continue; }
				uint64_t first = 0;
				kwage_group *g = load_file(ctx, files[fi], first);
				try{
					const uint64_t span = kwage_group_column_span(g);
					const uint32_t nf = files[fi].header.num_filter;
					column_bits.resize(std::max<uint64_t>(span, 1));
					check(kwage_group_column_bits(g, column_bits.data()));
					for(const SourceSet &s : sets){
						if(!same_params(files[s.file].header, files[fi].header)){ continue; }
						part.resize(std::max<uint64_t>(s.queries.size()*span, 1));
						check(kwage_search_filter_scores(g, s.fs, part.data(), span, 0, nullptr));
						for(size_t i = 0; i < s.queries.size(); ++i){
							QuerySample &qs = queries[s.queries[i]];
							for(uint32_t c = 0; c < nf; ++c){
								const uint64_t shared = part[i*span + first + c], sample_bits = column_bits[first + c];
								const uint64_t either = (uint64_t)qs.bits + sample_bits - shared;
								qs.best.push_back(Near{either ? (double)shared/(double)either : 0.0, (uint32_t)fi, c, (uint32_t)shared, (uint32_t)sample_bits});
							}
							const size_t keep = std::min<size_t>(k, qs.best.size());
							partial_sort(qs.best.begin(), qs.best.begin() + (long)keep, qs.best.end(), nearer);
							qs.best.resize(keep);
						}
					}
				}
				catch(...){ kwage_group_destroy(g); throw; }
				kwage_group_destroy(g);
			}
		}
		catch(...){
			for(SourceSet &s : sets){ kwage_filterset_destroy(s.fs); }
			kwage_shutdown(ctx);
			throw;
		}
		for(SourceSet &s : sets){ kwage_filterset_destroy(s.fs); }
		kwage_shutdown(ctx);

		TextSink to(out);
		to.put("query\trank\tsample\tshared_bits\tquery_bits\tsample_bits\tjaccard\n");
		for(const QuerySample &qs : queries){
			for(size_t r = 0; r < qs.best.size(); ++r){
				const Near &n = qs.best[r];
				char jac[32];
				snprintf(jac, sizeof(jac), "%.6f", n.jaccard);
				to.put(qs.accession); to.put('\t'); to.put((uint64_t)(r + 1)); to.put('\t'); to.put(names[n.file][n.column]);
				to.put('\t'); to.put((uint64_t)n.shared); to.put('\t'); to.put((uint64_t)qs.bits); to.put('\t'); to.put((uint64_t)n.sample_bits);
				to.put('\t'); to.put(jac); to.put('\n');
				to.drain();
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
