// kwage_amd/csrc/top_common.hpp -- what the top-k programs share (kwage_top, kwage_top_node): their command line (kwage's
// flags plus a required -k; -t defaults to 0) with its usage text, and the order in which a query's best samples are
// chosen.  Included after cli_common.hpp, whose read_command_line reads what TOP_CLI describes.
#ifndef KWAGE_AMD_TOP_COMMON_HPP
#define KWAGE_AMD_TOP_COMMON_HPP

#include "cli_common.hpp"

namespace {

const CliSpec TOP_CLI = {
	{
		"Usage for kwage_top (the k best-scoring samples per query):",
		"\t-k <number of samples per query> (1 to 1024)",
		"\t[-o <output file>] (default is stdout)",
		"\t[--o.csv (output CSV) | --o.json (output JSON)]",
		"\t[-t <search threshold>] (default is 0: the k best, whatever their score)",
		"\t-d <database search path> (can be repeated)",
		"\t[-i <input sequence file>] (can be repeated)",
		"\t[<DNA sequence>] (can be repeated)",
	},
	"odit", true,                                       // every flag of FLAG_TABLE
	true, nullptr, false,                               // a required -k (without a value it is a -k complaint, not usage); no -s
	0.0f, true, false,                                  // -t: 0 unless given, [0, 1]
	EXIT_FAILURE, EXIT_SUCCESS, EXIT_FAILURE,
	{BAD_K, BAD_THRESHOLD, BAD_QUERY_NAME, NO_QUERY, WALK_DB, NO_DB},
};
static_assert(KWAGE_TOPK_MAX == 1024u, "TOP_CLI's usage text quotes the cap");

// (score descending, file order, column ascending): the order in which a query's best samples are chosen
bool better(const Match &a, const Match &b)
{
	if(a.num_kmers_found != b.num_kmers_found){ return a.num_kmers_found > b.num_kmers_found; }
	return (a.file_index != b.file_index) ? (a.file_index < b.file_index) : (a.column < b.column);
}

}  // namespace

#endif
