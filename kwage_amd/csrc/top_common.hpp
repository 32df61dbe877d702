// kwage_amd/csrc/top_common.hpp -- what the top-k programs share (kwage_top, kwage_top_node): the usage text, the -k
// parser, the command line (kwage's flags plus -k; -t defaults to 0) and the order in which a query's best samples are
// chosen.  Included after cli_common.hpp.
#ifndef KWAGE_AMD_TOP_COMMON_HPP
#define KWAGE_AMD_TOP_COMMON_HPP

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

}  // namespace

#endif
