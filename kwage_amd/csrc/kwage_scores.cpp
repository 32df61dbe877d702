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
// Environment: KWAGE_DEVICE, KWAGE_BATCH_BASES (file_search.hpp).
#include "file_search.hpp"

namespace {

// kwage's -o, -d, -i and -h; anything else (-t, -k, the report formats) shows the usage text
const CliSpec SCORES_CLI = {
	{
		"Usage for kwage_scores (every query's match count for every sample, tab-separated):",
		"\t[-o <output file>] (default is stdout)",
		"\t-d <database search path> (can be repeated)",
		"\t[-i <input sequence file>] (can be repeated)",
		"\t[<DNA sequence>] (can be repeated)",
		"\t(the whole matrix, queries x samples x 4 bytes, is held in host memory until it is printed)",
	},
	"odi", false,
	false, nullptr, false,                              // no -k, no -s
	1.0f, false, false,                                 // (no -t)
	EXIT_FAILURE, EXIT_FAILURE, EXIT_FAILURE,
	{BAD_QUERY_NAME, NO_QUERY, WALK_DB, NO_DB},
};

// A batch's block of the matrix: one row per query, the files' real columns side by side.
struct Block {
	vector<uint32_t> nkmer;             // per query, for the k-mer length of the database's first file
	vector<uint32_t> cells;             // [query][sample]
};
typedef ResidentBatch<Block> Batch;

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(SCORES_CLI, argc, argv, cli, db_paths);
		if(status >= 0){ return status; }
		ofstream fout;
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;
		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, &infos);
		const uint64_t samples = place_samples(files);

		deque<Batch> batches;
		const bool fits = read_queries(cli, batches, [&](Batch &rb) {
			rb.kept.nkmer.assign(rb.q.size(), 0);
			return zeroed_block(rb.kept.cells, rb.q.size()*samples, samples, "x 4 bytes");
		});
		if(!fits){ return EXIT_FAILURE; }
		// ---- file by file: the file's matrix, its real columns copied to their place in each batch's block ---------------
		vector<uint32_t> part;
		search_file_by_file(files, batches, [&](size_t fi, const FileGroup &g, Batch &rb) {
			const uint64_t span = kwage_group_column_span(g.get());
			part.resize(std::max<uint64_t>(rb.q.size()*span, 1));
			check(kwage_search_scores(g.get(), rb.b, part.data(), span, fi == 0 ? rb.kept.nkmer.data() : nullptr, 0, nullptr));
			for(size_t q = 0; q < rb.q.size(); ++q){
				memcpy(rb.kept.cells.data() + q*samples + files[fi].first_column, part.data() + q*span + g.first, (size_t)g.nf*sizeof(uint32_t));
			}
		});

		// ---- the matrix: header, then the queries in kwage's order (the batches were made in that order) -------------------
		TextSink to(out);
		put_matrix_header(to, "query\tnum_kmers", files, infos);
		for(const Batch &rb : batches){
			for(size_t q = 0; q < rb.q.size(); ++q){
				put_query_name(to, rb, q);
				to.put('\t'); to.put((uint64_t)rb.kept.nkmer[q]);
				for(uint64_t c = 0; c < samples; ++c){ to.put('\t'); to.put((uint64_t)rb.kept.cells[q*samples + c]); to.drain(); }
				to.put('\n');
			}
		}
		to.flush();
		out.flush();
		return EXIT_SUCCESS;
	});
}
