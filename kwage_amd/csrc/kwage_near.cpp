// kwage_amd/csrc/kwage_near.cpp -- the `kwage_near` command-line program: for samples of the database, named by run
// accession, the k samples whose Bloom filters are most like theirs, by Jaccard index of the set rows (the filter search,
// kwage_search_filter_scores).  No counterpart in the reference.  The options are kwage's -d and -o, -k (default 10) and
// the accessions, positional or with -s (cli_common.hpp's reader).
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
// Environment: KWAGE_DEVICE (file_search.hpp).
#include "file_search.hpp"

namespace {

// kwage's -o, -d and -h, plus -k and -s; anything else shows the usage text
const CliSpec NEAR_CLI = {
	{
		"Usage for kwage_near (the samples most like given samples of the database, by Jaccard index of their Bloom filters):",
		"\t[-k <number of samples per query sample>] (1 to 1024, default is 10)",
		"\t[-o <output file>] (default is stdout)",
		"\t-d <database search path> (can be repeated)",
		"\t[-s <run accession>] (can be repeated)",
		"\t[<run accession>] (can be repeated)",
	},
	"od", false,
	true, "10", true,                                   // -k, 10 unless given; -s
	1.0f, false, false,                                 // (no -t)
	EXIT_FAILURE, EXIT_FAILURE, EXIT_FAILURE,
	{BAD_K, NO_ACCESSION, WALK_DB, NO_DB},
};
static_assert(KWAGE_TOPK_MAX == 1024u, "NEAR_CLI's usage text quotes the cap");

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

// The sets' row lists on the device, destroyed with this object.
struct SetsOnDevice {
	vector<SourceSet> &sets;
	~SetsOnDevice() { for(SourceSet &s : sets){ kwage_filterset_destroy(s.fs); } }
};

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(NEAR_CLI, argc, argv, cli, db_paths);
		if(status >= 0){ return status; }
		const uint32_t k = cli.k;
		const vector<string> &accessions = cli.accessions;

		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, &infos);
		vector<vector<string>> names(db_paths.size());          // run accession of every column
		for(size_t i = 0; i < files.size(); ++i){
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
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;

		{
			Device device;                              // (declared first: shut down last)
			SetsOnDevice on_device{sets};
			// ---- first pass: the source files, their query samples' row lists kept on the device -----------------------------
			for(SourceSet &s : sets){
				const FileGroup g(device.ctx, files[s.file]);
				vector<uint64_t> cols;
				for(uint32_t q : s.queries){ cols.push_back(g.first + queries[q].column); }
				check(kwage_filterset_from_columns(g.get(), cols.data(), (uint32_t)cols.size(), &s.fs));
				vector<uint32_t> bits(cols.size());
				check(kwage_filterset_bit_counts(s.fs, bits.data()));
				for(size_t i = 0; i < cols.size(); ++i){ queries[s.queries[i]].bits = bits[i]; }
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
				const FileGroup g(device.ctx, files[fi]);
				const uint64_t span = kwage_group_column_span(g.get()), first = g.first;
				const uint32_t nf = files[fi].header.num_filter;
				column_bits.resize(std::max<uint64_t>(span, 1));
				check(kwage_group_column_bits(g.get(), column_bits.data()));
				for(const SourceSet &s : sets){
					if(!same_params(files[s.file].header, files[fi].header)){ continue; }
					part.resize(std::max<uint64_t>(s.queries.size()*span, 1));
					check(kwage_search_filter_scores(g.get(), s.fs, part.data(), span, 0, nullptr));
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
		}

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
		return EXIT_SUCCESS;
	});
}
