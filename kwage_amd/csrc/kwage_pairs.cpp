// kwage_amd/csrc/kwage_pairs.cpp -- the `kwage_pairs` command-line program: the shared set bits of every pair of samples
// of the database -- or their Jaccard index -- as a tab-separated matrix (the overlap matrix, kwage_group_column_overlaps:
// an integer matrix product on the matrix cores).  No counterpart in the reference.  The options are kwage's -d and -o,
// the samples by run accession, positional or with -s (cli_common.hpp's reader; none: every sample), and --jaccard.
//
//   sample <TAB> accession ... <TAB> accession
//   accession <TAB> cell ... <TAB> cell            one line per sample, in the header's order
//
// A cell is the number of rows set in both samples' Bloom filters -- on the diagonal the sample's own set bits -- or, with
// --jaccard, shared / (bits_i + bits_j - shared) as a double (0 where that is empty), printed with %.6f.
//
// An accession is the first (file, column) carrying it, in database order; one found nowhere ends the program with a
// message that names it, before a device is opened.  One group per file; the file pairs i <= j are gone through with two
// groups resident at a time: file i against itself in the symmetric form, then against every later file in the a x b
// form, mirrored on the host.  Files whose Bloom parameters differ from the first sample's are skipped with one line on
// stderr: filters built differently are not comparable.
//
// Environment: KWAGE_DEVICE (file_search.hpp).
#include "file_search.hpp"

namespace {

// kwage's -o, -d and -h, plus -s; anything else shows the usage text (--jaccard is taken out beforehand)
const CliSpec PAIRS_CLI = {
	{
		"Usage for kwage_pairs (the shared set bits of every pair of samples of the database, or their Jaccard index):",
		"\t[-o <output file>] (default is stdout)",
		"\t[--jaccard] (Jaccard index instead of shared bits)",
		"\t-d <database search path> (can be repeated)",
		"\t[-s <run accession>] (can be repeated; default is every sample)",
		"\t[<run accession>] (can be repeated)",
	},
	"od", false,
	false, nullptr, true,                               // no -k; -s
	1.0f, false, false,                                 // (no -t)
	EXIT_FAILURE, EXIT_FAILURE, EXIT_FAILURE,
	{WALK_DB, NO_DB},
};

struct Sample {
	string accession;
	uint32_t file = 0, column = 0;
};

bool same_params(const kwage_db_header &a, const kwage_db_header &b)
{
	return a.kmer_len == b.kmer_len && a.num_hash == b.num_hash && a.log_2_filter_len == b.log_2_filter_len && a.hash_func == b.hash_func;
}

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		// --jaccard is this program's own: the shared reader sees the command line without it
		bool jaccard = false;
		vector<char*> args;
		for(int i = 0; i < argc; ++i){
			if(i > 0 && !strcmp(argv[i], "--jaccard")){ jaccard = true; }
			else{ args.push_back(argv[i]); }
		}
		args.push_back(nullptr);
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(PAIRS_CLI, (int)args.size() - 1, args.data(), cli, db_paths);
		if(status >= 0){ return status; }

		vector<DbFileEntry> files;
		vector<DbInfo> infos;
		read_database_files(db_paths, files, &infos);
		vector<Sample> all;
		for(size_t fi = 0; fi < files.size(); ++fi){
			for(uint32_t c = 0; c < files[fi].header.num_filter; ++c){
				FilterInfo info;
				if(!infos[fi].info(c, info)){ throw "binary_read<FilterInfo>: Unable to read FilterInfo"; }
				all.push_back(Sample{info.csv_string(), (uint32_t)fi, c});
			}
		}
		vector<Sample> samples;
		if(cli.accessions.empty()){ samples = all; }
		for(const string &acc : cli.accessions){
			const auto at = find_if(all.begin(), all.end(), [&](const Sample &s) { return s.accession == acc; });
			if(at == all.end()){
				cerr << "No sample with the run accession " << acc << " in the database" << endl;
				return EXIT_FAILURE;
			}
			samples.push_back(*at);
		}
		if(samples.empty()){
			cerr << "The database holds no sample" << endl;
			return EXIT_FAILURE;
		}
		// files built differently from the first sample's are left out, their samples with them
		const kwage_db_header &want = files[samples[0].file].header;
		for(size_t fi = 0; fi < files.size(); ++fi){
			const bool used = any_of(samples.begin(), samples.end(), [&](const Sample &s) { return s.file == fi; });
			if(used && !same_params(files[fi].header, want)){
				cerr << "Skipping " << files[fi].path << ": its Bloom filter parameters differ from those of " << samples[0].accession << endl;
			}
		}
		samples.erase(remove_if(samples.begin(), samples.end(), [&](const Sample &s) { return !same_params(files[s.file].header, want); }), samples.end());
		const size_t n = samples.size();
		// per file the places of its samples in the matrix, in list order
		vector<vector<size_t>> of_file(files.size());
		for(size_t i = 0; i < n; ++i){ of_file[samples[i].file].push_back(i); }
		vector<size_t> used;
		for(size_t fi = 0; fi < files.size(); ++fi){ if(!of_file[fi].empty()){ used.push_back(fi); } }

		ofstream fout;
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;

		vector<uint32_t> matrix;
		try{ matrix.assign(n*n, 0); }
		catch(const std::bad_alloc&){
			cerr << "The matrix does not fit in host memory: " << n << " x " << n << " samples" << endl;
			return EXIT_FAILURE;
		}
		{
			Device device;                              // (declared first: shut down last)
			vector<uint32_t> cells;
			for(size_t x = 0; x < used.size(); ++x){
				const size_t fa = used[x];
				const FileGroup ga(device.ctx, files[fa]);
				vector<uint64_t> ca;
				for(size_t i : of_file[fa]){ ca.push_back(ga.first + samples[i].column); }
				cells.assign(ca.size()*ca.size(), 0);
				check(kwage_group_column_overlaps(ga.get(), ca.data(), (uint32_t)ca.size(), nullptr, nullptr, 0, cells.data(), ca.size(), 0, nullptr));
				for(size_t i = 0; i < ca.size(); ++i){
					for(size_t j = 0; j < ca.size(); ++j){ matrix[of_file[fa][i]*n + of_file[fa][j]] = cells[i*ca.size() + j]; }
				}
				for(size_t y = x + 1; y < used.size(); ++y){
					const size_t fb = used[y];
					const FileGroup gb(device.ctx, files[fb]);
					vector<uint64_t> cb;
					for(size_t j : of_file[fb]){ cb.push_back(gb.first + samples[j].column); }
					cells.assign(ca.size()*cb.size(), 0);
					check(kwage_group_column_overlaps(ga.get(), ca.data(), (uint32_t)ca.size(), gb.get(), cb.data(), (uint32_t)cb.size(), cells.data(), cb.size(), 0, nullptr));
					for(size_t i = 0; i < ca.size(); ++i){
						for(size_t j = 0; j < cb.size(); ++j){
							matrix[of_file[fa][i]*n + of_file[fb][j]] = matrix[of_file[fb][j]*n + of_file[fa][i]] = cells[i*cb.size() + j];
						}
					}
				}
			}
		}

		TextSink to(out);
		to.put("sample");
		for(const Sample &s : samples){ to.put('\t'); to.put(s.accession); to.drain(); }
		to.put('\n');
		for(size_t i = 0; i < n; ++i){
			to.put(samples[i].accession);
			for(size_t j = 0; j < n; ++j){
				to.put('\t');
				const uint64_t shared = matrix[i*n + j];
				if(jaccard){
					const uint64_t either = (uint64_t)matrix[i*n + i] + matrix[j*n + j] - shared;
					char jac[32];
					snprintf(jac, sizeof(jac), "%.6f", either ? (double)shared/(double)either : 0.0);
					to.put(jac);
				}
				else{ to.put(shared); }
				to.drain();
			}
			to.put('\n');
		}
		to.flush();
		out.flush();
		return EXIT_SUCCESS;
	});
}
