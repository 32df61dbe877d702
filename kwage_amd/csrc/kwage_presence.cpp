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
// Environment: KWAGE_DEVICE, KWAGE_BATCH_BASES (file_search.hpp).
#include "file_search.hpp"

namespace {

// kwage's -o, -t, -d, -i and -h; anything else (-k, the report formats) shows the usage text
const CliSpec PRESENCE_CLI = {
	{
		"Usage for kwage_presence (which samples hold each query: a tab-separated 0/1 matrix):",
		"\t[-o <output file>] (default is stdout)",
		"\t[-t <search threshold>] (default is 1)",
		"\t-d <database search path> (can be repeated)",
		"\t[-i <input sequence file>] (can be repeated)",
		"\t[<DNA sequence>] (can be repeated)",
		"\t(the whole matrix, samples / 8 bytes per query, is held in host memory until it is printed)",
	},
	"odit", false,
	false, nullptr, false,                              // no -k, no -s
	1.0f, false, false,                                 // -t: 1 unless given, (0, 1]
	EXIT_FAILURE, EXIT_FAILURE, EXIT_FAILURE,
	{BAD_THRESHOLD, BAD_QUERY_NAME, NO_QUERY, WALK_DB, NO_DB},
};

// A batch's block of the matrix: one row of row_bytes per query, bit s = sample s.
struct Block {
	vector<uint32_t> nkmer;             // per query, for the k-mer length of the database's first file
	vector<uint32_t> passing;           // per query, summed over the files
	vector<uint8_t> bits;               // [query][row_bytes]
};
typedef ResidentBatch<Block> Batch;

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(PRESENCE_CLI, argc, argv, cli, db_paths);
		if(status >= 0){ return status; }
		ofstream fout;
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;
		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, &infos);
		const uint64_t samples = place_samples(files);
		const uint64_t row_bytes = (samples + 7)/8;

		deque<Batch> batches;
		const bool fits = read_queries(cli, batches, [&](Batch &rb) {
			rb.kept.nkmer.assign(rb.q.size(), 0);
			rb.kept.passing.assign(rb.q.size(), 0);
			return zeroed_block(rb.kept.bits, rb.q.size()*row_bytes, samples, "/ 8 bytes");
		});
		if(!fits){ return EXIT_FAILURE; }
		// ---- file by file: the file's bitmap, its real columns copied to their place in each batch's block ---------------
		vector<uint8_t> part;
		vector<uint32_t> passing;
		search_file_by_file(files, batches, [&](size_t fi, const FileGroup &g, Batch &rb) {
			const uint64_t w = (kwage_group_row_bytes(g.get()) + 15)/16*16;
			part.resize(std::max<uint64_t>(rb.q.size()*w, 1));
			passing.assign(std::max<size_t>(rb.q.size(), 1), 0);
			check(kwage_search_presence(g.get(), rb.b, cli.threshold, part.data(), w, passing.data(), fi == 0 ? rb.kept.nkmer.data() : nullptr, KWAGE_SEARCH_EARLY_EXIT, nullptr));
			for(size_t q = 0; q < rb.q.size(); ++q){
				rb.kept.passing[q] += passing[q];
				if(!passing[q]){ continue; }
				const uint8_t *src = part.data() + q*w;
				uint8_t *dst = rb.kept.bits.data() + q*row_bytes;
				for(uint64_t c = 0; c < g.nf; ++c){
					const uint64_t from = g.first + c, to = files[fi].first_column + c;
					if((src[from >> 3] >> (from & 7)) & 1u){ dst[to >> 3] |= (uint8_t)(1u << (to & 7)); }
				}
			}
		});

		// ---- the matrix: header, then the queries in kwage's order (the batches were made in that order) -------------------
		TextSink to(out);
		put_matrix_header(to, "query\tnum_kmers\tpassing", files, infos);
		for(const Batch &rb : batches){
			for(size_t q = 0; q < rb.q.size(); ++q){
				put_query_name(to, rb, q);
				to.put('\t'); to.put((uint64_t)rb.kept.nkmer[q]);
				to.put('\t'); to.put((uint64_t)rb.kept.passing[q]);
				const uint8_t *row = rb.kept.bits.data() + q*row_bytes;
				for(uint64_t c = 0; c < samples; ++c){ to.put('\t'); to.put((row[c >> 3] >> (c & 7)) & 1u ? '1' : '0'); to.drain(); }
				to.put('\n');
			}
		}
		to.flush();
		out.flush();
		return EXIT_SUCCESS;
	});
}
