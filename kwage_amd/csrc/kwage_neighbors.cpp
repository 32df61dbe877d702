// kwage_amd/csrc/kwage_neighbors.cpp -- the `kwage_neighbors` command-line program: for samples of the database -- every
// sample unless some are named -- the k samples whose Bloom filters are most like theirs, by Jaccard index or by shared set
// bits, chosen on the device (kwage_group_column_neighbors: the overlap matrix's cells, reduced strip by strip to k records
// per sample, so that the n x n matrix exists nowhere).  No counterpart in the reference.  The options are kwage's -d and
// -o, -k, the samples by run accession, positional or with -s (cli_common.hpp's reader; none: every sample), --shared
// and --min-shared <n>.
//
//   sample <TAB> neighbour <TAB> rank <TAB> shared <TAB> bits_sample <TAB> bits_neighbour <TAB> jaccard
//
// One line per neighbour, per sample in list order, best first, ranks from 1; jaccard = shared / (bits_sample +
// bits_neighbour - shared) as a double (0 where that is empty), printed with %.6f.  The order is exact: by the fraction
// (or, with --shared, by the shared bits), then by the neighbour's place in the database (file, column).  A sample is
// never its own neighbour.  --min-shared leaves out neighbours that share fewer bits.
//
// An accession is the first (file, column) carrying it, in database order; one found nowhere ends the program with a
// message that names it, before a device is opened.  One group per file, two resident at a time as in kwage_pairs: a file
// against itself once, a pair of files x < y in both directions (the named samples restrict the querying side only), a
// sample's running list of k merged on the host after every call -- host memory is O(n k).  Files whose Bloom parameters
// differ from the first sample's are skipped with one line on stderr: filters built differently are not comparable.
//
// Environment: KWAGE_DEVICE (file_search.hpp).
#include "file_search.hpp"

namespace {

// kwage's -o, -d and -h, plus -k and -s; anything else shows the usage text (--shared and --min-shared are taken out beforehand)
const CliSpec NEIGHBORS_CLI = {
	{
		"Usage for kwage_neighbors (each sample's k most similar samples of the database, by Jaccard index of their Bloom filters):",
		"\t-k <number of neighbours per sample> (1 to 1024)",
		"\t[-o <output file>] (default is stdout)",
		"\t[--shared] (order by shared bits instead of the Jaccard index)",
		"\t[--min-shared <n>] (leave out neighbours sharing fewer bits; default is 0)",
		"\t-d <database search path> (can be repeated)",
		"\t[-s <run accession>] (can be repeated; default is every sample)",
		"\t[<run accession>] (can be repeated)",
	},
	"od", false,
	true, nullptr, true,                                // a required -k; -s
	1.0f, false, false,                                 // (no -t)
	EXIT_FAILURE, EXIT_FAILURE, EXIT_FAILURE,
	{BAD_K, WALK_DB, NO_DB},
};
static_assert(KWAGE_TOPK_MAX == 1024u, "NEIGHBORS_CLI's usage text quotes the cap");

struct Sample {
	string accession;
	uint32_t file = 0, column = 0;
};

// A neighbour of a running list: the record and where its sample stands in the database.
struct Near {
	uint32_t shared = 0, bits_a = 0, bits_b = 0;
	uint32_t file = 0, column = 0;
};

bool same_params(const kwage_db_header &a, const kwage_db_header &b)
{
	return a.kmer_len == b.kmer_len && a.num_hash == b.num_hash && a.log_2_filter_len == b.log_2_filter_len && a.hash_func == b.hash_func;
}

// The exact order of the call, then the database's: x before y.
bool before(const Near &x, const Near &y, bool by_shared)
{
	if(by_shared){
		if(x.shared != y.shared){ return x.shared > y.shared; }
	}
	else{
		// shared / union as fractions (an empty union counts as 0): both products are below 2^64
		const uint64_t ux = (uint64_t)x.bits_a + x.bits_b - x.shared, uy = (uint64_t)y.bits_a + y.bits_b - y.shared;
		const unsigned __int128 l = (unsigned __int128)(ux ? x.shared : 0)*(uy ? uy : 1), r = (unsigned __int128)(uy ? y.shared : 0)*(ux ? ux : 1);
		if(l != r){ return l > r; }
	}
	return x.file != y.file ? x.file < y.file : x.column < y.column;
}

}  // namespace

int main(int argc, char *argv[])
{
	return guarded([&]() -> int {
		// --shared and --min-shared are this program's own: the shared reader sees the command line without them
		bool by_shared = false;
		uint32_t min_shared = 0;
		vector<char*> args;
		for(int i = 0; i < argc; ++i){
			if(i > 0 && !strcmp(argv[i], "--shared")){ by_shared = true; }
			else if(i > 0 && !strcmp(argv[i], "--min-shared")){
				char *end = nullptr;
				const unsigned long long v = i + 1 < argc ? strtoull(argv[i + 1], &end, 10) : 0;
				if(i + 1 >= argc || !*argv[i + 1] || *end || argv[i + 1][0] == '-' || v > 0xFFFFFFFFull){
					cerr << "Please provide: 0 <= --min-shared < 2^32" << endl;
					return EXIT_FAILURE;
				}
				min_shared = (uint32_t)v;
				++i;
			}
			else{ args.push_back(argv[i]); }
		}
		args.push_back(nullptr);
		Cli cli;
		vector<string> db_paths;
		const int status = read_command_line(NEIGHBORS_CLI, (int)args.size() - 1, args.data(), cli, db_paths);
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
			if(!same_params(files[fi].header, want)){
				cerr << "Skipping " << files[fi].path << ": its Bloom filter parameters differ from those of " << samples[0].accession << endl;
			}
		}
		samples.erase(remove_if(samples.begin(), samples.end(), [&](const Sample &s) { return !same_params(files[s.file].header, want); }), samples.end());
		const size_t n = samples.size();
		// per file the places of its querying samples, in list order; the candidate files
		vector<vector<size_t>> of_file(files.size());
		for(size_t i = 0; i < n; ++i){ of_file[samples[i].file].push_back(i); }
		vector<size_t> used;
		for(size_t fi = 0; fi < files.size(); ++fi){ if(same_params(files[fi].header, want) && files[fi].header.num_filter){ used.push_back(fi); } }
		// a sample's accession by (file, column)
		vector<size_t> first_of(files.size() + 1, 0);
		for(size_t fi = 0; fi < files.size(); ++fi){ first_of[fi + 1] = first_of[fi] + files[fi].header.num_filter; }

		ofstream fout;
		if(!open_output(cli.output_path, fout)){ return EXIT_FAILURE; }
		ostream &out = fout.is_open() ? fout : cout;

		const uint32_t k = cli.k;
		const uint32_t metric = by_shared ? KWAGE_NEIGHBORS_SHARED : KWAGE_NEIGHBORS_JACCARD;
		vector<vector<Near>> lists(n);
		{
			Device device;                              // (declared first: shut down last)
			vector<kwage_neighbor> records;
			vector<uint32_t> counts;
			// the querying samples of file fq (group gq) against every sample of file fc (group gc)
			auto run = [&](size_t fq, const FileGroup &gq, size_t fc, const FileGroup &gc) {
				const vector<size_t> &who = of_file[fq];
				if(who.empty()){ return; }
				vector<uint64_t> ca, cb;
				for(size_t i : who){ ca.push_back(gq.first + samples[i].column); }
				for(uint32_t c = 0; c < gc.nf; ++c){ cb.push_back(gc.first + c); }
				records.assign(ca.size()*(size_t)k, kwage_neighbor{});
				counts.assign(ca.size(), 0);
				check(kwage_group_column_neighbors(gq.get(), ca.data(), (uint32_t)ca.size(), gc.get(), cb.data(), (uint32_t)cb.size(), k, metric, min_shared,
				                                   records.data(), counts.data(), KWAGE_NEIGHBORS_SKIP_SELF, nullptr));
				for(size_t q = 0; q < who.size(); ++q){
					vector<Near> &list = lists[who[q]];
					for(uint32_t r = 0; r < counts[q]; ++r){
						const kwage_neighbor &rec = records[q*k + r];
						list.push_back(Near{rec.shared, rec.bits_a, rec.bits_b, (uint32_t)fc, rec.index});
					}
					stable_sort(list.begin(), list.end(), [&](const Near &x, const Near &y) { return before(x, y, by_shared); });
					if(list.size() > k){ list.resize(k); }
				}
			};
			for(size_t x = 0; x < used.size(); ++x){
				const size_t fa = used[x];
				const bool later = any_of(used.begin() + x + 1, used.end(), [&](size_t f) { return !of_file[f].empty(); });
				if(of_file[fa].empty() && !later){ continue; }
				const FileGroup ga(device.ctx, files[fa]);
				run(fa, ga, fa, ga);
				for(size_t y = x + 1; y < used.size(); ++y){
					const size_t fb = used[y];
					if(of_file[fa].empty() && of_file[fb].empty()){ continue; }
					const FileGroup gb(device.ctx, files[fb]);
					run(fa, ga, fb, gb);
					run(fb, gb, fa, ga);
				}
			}
		}

		TextSink to(out);
		to.put("sample\tneighbour\trank\tshared\tbits_sample\tbits_neighbour\tjaccard\n");
		for(size_t i = 0; i < n; ++i){
			for(size_t r = 0; r < lists[i].size(); ++r){
				const Near &v = lists[i][r];
				to.put(samples[i].accession);
				to.put('\t'); to.put(all[first_of[v.file] + v.column].accession);
				to.put('\t'); to.put((uint64_t)(r + 1));
				to.put('\t'); to.put((uint64_t)v.shared);
				to.put('\t'); to.put((uint64_t)v.bits_a);
				to.put('\t'); to.put((uint64_t)v.bits_b);
				const uint64_t either = (uint64_t)v.bits_a + v.bits_b - v.shared;
				char jac[32];
				snprintf(jac, sizeof(jac), "\t%.6f\n", either ? (double)v.shared/(double)either : 0.0);
				to.put(jac);
				to.drain();
			}
		}
		to.flush();
		out.flush();
		return EXIT_SUCCESS;
	});
}
