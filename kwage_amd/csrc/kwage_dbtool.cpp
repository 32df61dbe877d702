// kwage_amd/csrc/kwage_dbtool.cpp -- command-line front end to the database-side entry points of the C ABI
// (include/kwage_amd.h): what the reference spreads over dump_db / merge_db / the build_db step of maestro.
//
//   kwage_dbtool info <file.db|.dbz>                                header fields (dump_db.cpp:150-200 prints the same)
//   kwage_dbtool accessions <file.db|.dbz>                          run accession of every column
//   kwage_dbtool compress <in.db> <out.dbz> [threads]               raw -> deflate container (host)
//   kwage_dbtool decompress <in.dbz> <out.db>                       container -> raw (host)
//   kwage_dbtool build <out.db> <k> <log2 len> <num hash> <f.bloom>...   .bloom files -> .db   (device bit transpose)
//   kwage_dbtool repack <out.db> <in.db>...                         same-parameter files -> one wide file (device)
//   kwage_dbtool append <out.db> <in.db> <x.bloom>...               in.db loaded into a group, the filters inserted live behind it
//                                                                   (kwage_group_insert_bloom_files), everything saved as one
//                                                                   file (kwage_group_save_db): what `build` makes of all the
//                                                                   `.bloom` files, without the ones in.db was built from
//   kwage_dbtool drop <out.db> <in.db> <run accession>...           in.db without the listed samples; exit code 1 when one of
//                                                                   them is not in the file
//   kwage_dbtool extract <out dir> <in.db> [<run accession>...]     in.db loaded into a group, the named samples (none named:
//                                                                   all, in column order) written back as the `.bloom` files
//                                                                   they were built from, <out dir>/<accession>.bloom
//                                                                   (kwage_group_export_bloom_files), records copied verbatim;
//                                                                   exit code 1, nothing written, when one is not in the file
//   kwage_dbtool fold <out.db> <in.db|.dbz> <log2 len>            in.db loaded into a group, its Bloom filters shortened to
//                                                                   2^<log2 len> bits on the device (kwage_group_fold), all
//                                                                   columns saved with their records copied verbatim: byte for
//                                                                   byte what `build` makes of the same filters built at that
//                                                                   length.  stderr: the share of set bits per column before
//                                                                   and after and the false-positive rate it buys; exit code 1,
//                                                                   nothing written, for a length not below the file's
//   kwage_dbtool union <out.db> <in.db> <NEW>=<ACC1>,<ACC2>[,...]...  in.db loaded into a group, per argument one new column, the OR
//                                                                   of the named samples' columns made on the device
//                                                                   (kwage_group_union_columns): the Bloom filter of their reads
//                                                                   together.  Everything saved as one file; members keep their
//                                                                   records, a new column gets its run accession <NEW> and no
//                                                                   other field.  stderr: per new column the bits set and the
//                                                                   false-positive rate fill^num_hash; exit code 1, nothing
//                                                                   written, when a member is not in the file
//   kwage_dbtool merge <out.db> <in.db> <NEW>=<ACC1>,<ACC2>[,...]...  the same, with the members dropped from the output
//   kwage_dbtool mkbloom <out.bloom> <accession> <k> <log2 len|0> <num hash|0> <seq file> [p]
//                                                                   exact k-mer set of a FASTA/FASTQ -> .bloom; 0 0 = pick the
//                                                                   parameters with optimal_bloom_param(p, default 0.25)
//   kwage_dbtool countbloom <out.bloom> <accession> <k> <min count> <seq file>... [-p p] [-l min log2] [-L max log2]
//                                                                   make_bloom_filter() with a minimum k-mer count (reference
//                                                                   default 5): counting filters sized from the number of bases,
//                                                                   parameters from optimal_bloom_param; exit code 3 = INVALID
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "kwage_amd.h"

static int die(const char *what)
{
	fprintf(stderr, "kwage_dbtool: %s: %s\n", what, kwage_last_error());
	return 1;
}

static int usage()
{
	fprintf(stderr,
		"usage: kwage_dbtool info|accessions <file>\n"
		"       kwage_dbtool compress <in.db> <out.dbz> [threads] | decompress <in.dbz> <out.db>\n"
		"       kwage_dbtool build <out.db> <k> <log2 len> <num hash> <f.bloom>...\n"
		"       kwage_dbtool repack <out.db> <in.db>...\n"
		"       kwage_dbtool append <out.db> <in.db> <x.bloom>...\n"
		"       kwage_dbtool drop <out.db> <in.db> <run accession>...\n"
		"       kwage_dbtool extract <out dir> <in.db> [<run accession>...]\n"
		"       kwage_dbtool fold <out.db> <in.db|.dbz> <log2 len>\n"
		"       kwage_dbtool union|merge <out.db> <in.db> <new accession>=<run accession>[,<run accession>...]...\n"
		"       kwage_dbtool mkbloom <out.bloom> <accession> <k> <log2 len|0> <num hash|0> <seq file> [p]\n"
		"       kwage_dbtool countbloom <out.bloom> <accession> <k> <min count> <seq file>... [-p p] [-l min log2] [-L max log2]\n");
	return 2;
}

// in.db loaded into a fresh group with room for `extra` more columns behind it (on the next 16-byte boundary of the row).
static int load_db(kwage_ctx *ctx, const char *in_db, uint64_t extra, kwage_db_header *h, kwage_group **g)
{
	if(kwage_db_read_header(in_db, h)){ return die("read header"); }
	const kwage_params p = {h->kmer_len, h->num_hash, h->log_2_filter_len, h->hash_func};
	const uint64_t file_bytes = ((uint64_t)h->num_filter + 7)/8;
	if(kwage_group_create(ctx, &p, extra ? (file_bytes + 15)/16*16*8 + extra : file_bytes*8, g)){ return die("create group"); }
	uint64_t first = 0;
	uint32_t nf = 0;
	if(kwage_group_add_db_file(*g, in_db, &first, &nf)){ kwage_group_destroy(*g); *g = NULL; return die("load"); }
	return 0;
}

static int save_columns(kwage_group *g, const char *out_db, const std::vector<kwage_save_column> &cols)
{
	kwage_save_stats st;
	if(cols.empty() || cols.size() > 0xFFFFFFFFull){ fprintf(stderr, "kwage_dbtool: save: no column is left to write\n"); return 1; }
	if(kwage_group_save_db(g, out_db, cols.data(), (uint32_t)cols.size(), 0, &st)){ return die("save"); }
	fprintf(stderr, "wrote %s: %zu columns, %llu bytes, %llu runs, extract kernel %.3f ms\n", out_db, cols.size(), (unsigned long long)st.db_bytes,
	        (unsigned long long)st.runs, st.extract_kernel_ms);
	return 0;
}

static int append_blooms(kwage_ctx *ctx, const char *out_db, const char *in_db, const char *const *blooms, uint32_t n)
{
	kwage_db_header h;
	kwage_group *g = NULL;
	int rc = load_db(ctx, in_db, n, &h, &g);
	if(rc){ return rc; }
	uint64_t first = 0;
	if(kwage_group_insert_bloom_files(g, blooms, n, 0, &first, NULL)){ kwage_group_destroy(g); return die("insert"); }
	// the new columns' FilterInfo records are kwage_build_db's own: a side file of the new filters is built for them and
	// removed again (a `.bloom` file's record reaches the save verbatim through a `.db` file only)
	const std::string side = std::string(out_db) + ".records." + std::to_string((long long)getpid());
	const kwage_params p = {h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func};
	if(kwage_build_db(ctx, side.c_str(), &p, blooms, n, NULL)){ kwage_group_destroy(g); (void)remove(side.c_str()); return die("build"); }
	std::vector<kwage_save_column> cols;
	for(uint32_t j = 0; j < h.num_filter; ++j){ cols.push_back(kwage_save_column{j, in_db, j, NULL}); }
	for(uint32_t j = 0; j < n; ++j){ cols.push_back(kwage_save_column{first + j, side.c_str(), j, NULL}); }
	rc = save_columns(g, out_db, cols);
	(void)remove(side.c_str());
	kwage_group_destroy(g);
	return rc;
}

// The run accession of every column of in_db; every one of the n `accessions` must be among them (else exit code 1).
static int read_accessions(const char *what, const char *in_db, char **accessions, int n, std::vector<std::string> &have)
{
	kwage_dbinfo *d = NULL;
	if(kwage_dbinfo_open(in_db, &d)){ return die("read metadata"); }
	have.assign(kwage_dbinfo_num_filter(d), std::string());
	char buf[64];
	for(uint32_t j = 0; j < have.size(); ++j){
		if(kwage_dbinfo_csv_string(d, j, buf, sizeof(buf))){ kwage_dbinfo_close(d); return die("read FilterInfo"); }
		have[j] = buf;
	}
	kwage_dbinfo_close(d);
	for(int i = 0; i < n; ++i){
		bool found = false;
		for(const std::string &a : have){ found = found || a == accessions[i]; }
		if(!found){ fprintf(stderr, "kwage_dbtool: %s: %s holds no sample with run accession %s\n", what, in_db, accessions[i]); return 1; }
	}
	return 0;
}

static int drop_samples(kwage_ctx *ctx, const char *out_db, const char *in_db, char **accessions, int n)
{
	std::vector<std::string> have;
	int rc = read_accessions("drop", in_db, accessions, n, have);
	if(rc){ return rc; }
	kwage_db_header h;
	kwage_group *g = NULL;
	if((rc = load_db(ctx, in_db, 0, &h, &g))){ return rc; }
	std::vector<kwage_save_column> cols;
	for(uint32_t j = 0; j < have.size(); ++j){
		bool gone = false;
		for(int i = 0; i < n; ++i){ gone = gone || have[j] == accessions[i]; }
		if(!gone){ cols.push_back(kwage_save_column{j, in_db, j, NULL}); }
	}
	rc = save_columns(g, out_db, cols);
	kwage_group_destroy(g);
	return rc;
}

static int extract_samples(kwage_ctx *ctx, const char *out_dir, const char *in_db, char **accessions, int n)
{
	std::vector<std::string> have;
	int rc = read_accessions("extract", in_db, accessions, n, have);
	if(rc){ return rc; }
	// the named samples in the order named (the first column that carries the accession), or every column
	std::vector<kwage_save_column> cols;
	std::vector<std::string> paths;
	auto take = [&](uint32_t j) {
		cols.push_back(kwage_save_column{j, in_db, j, NULL});
		paths.push_back(std::string(out_dir) + "/" + have[j] + ".bloom");
	};
	if(n == 0){ for(uint32_t j = 0; j < have.size(); ++j){ take(j); } }
	for(int i = 0; i < n; ++i){
		for(uint32_t j = 0; j < have.size(); ++j){ if(have[j] == accessions[i]){ take(j); break; } }
	}
	if(cols.empty()){ fprintf(stderr, "kwage_dbtool: extract: %s holds no sample\n", in_db); return 1; }
	kwage_db_header h;
	kwage_group *g = NULL;
	if((rc = load_db(ctx, in_db, 0, &h, &g))){ return rc; }
	(void)mkdir(out_dir, 0777);                       // (it may exist)
	std::vector<const char*> out(paths.size());
	for(size_t i = 0; i < paths.size(); ++i){ out[i] = paths[i].c_str(); }
	float ms = 0;
	if(kwage_group_export_bloom_files(g, cols.data(), out.data(), (uint32_t)cols.size(), 0, KWAGE_SEARCH_TIMING, &ms)){ rc = die("extract"); }
	else{ fprintf(stderr, "wrote %zu .bloom files to %s, export kernel %.3f ms\n", cols.size(), out_dir, ms); }
	kwage_group_destroy(g);
	return rc;
}

// The mean and the largest share of set bits among the columns of a finalized group (kwage_group_column_bits over 2^L rows).
static int column_shares(kwage_group *g, uint32_t log_2_len, uint32_t num_filter, double *mean, double *largest)
{
	std::vector<uint32_t> bits(kwage_group_column_span(g), 0u);
	if(kwage_group_column_bits(g, bits.data())){ return die("column bits"); }
	const double rows = (double)(1ull << log_2_len);
	double sum = 0;
	uint32_t top = 0;
	for(uint32_t j = 0; j < num_filter; ++j){ sum += bits[j]; top = std::max(top, bits[j]); }
	*mean = sum/rows/(double)num_filter;
	*largest = (double)top/rows;
	return 0;
}

static int fold_db(kwage_ctx *ctx, const char *out_db, const char *in_db, uint32_t log_2_len)
{
	kwage_db_header h;
	if(kwage_db_read_header(in_db, &h)){ return die("read header"); }
	if(log_2_len >= h.log_2_filter_len){
		fprintf(stderr, "kwage_dbtool: fold: 2^%u is not below the file's filter length 2^%u\n", log_2_len, h.log_2_filter_len);
		return 1;
	}
	kwage_group *g = NULL, *folded = NULL;
	int rc = load_db(ctx, in_db, 0, &h, &g);
	if(rc){ return rc; }
	kwage_fold_stats st;
	if(kwage_group_fold(g, log_2_len, KWAGE_SEARCH_TIMING, &folded, &st)){ kwage_group_destroy(g); return die("fold"); }
	std::vector<kwage_save_column> cols;
	for(uint32_t j = 0; j < h.num_filter; ++j){ cols.push_back(kwage_save_column{j, in_db, j, NULL}); }
	rc = save_columns(folded, out_db, cols);
	// what the shorter filters cost: a query k-mer that is absent passes a column with probability share^num_hash
	double mean[2] = {0, 0}, largest[2] = {0, 0};
	if(!rc && (kwage_group_finalize(g) || kwage_group_finalize(folded))){ rc = die("finalize"); }
	if(!rc){ rc = column_shares(g, h.log_2_filter_len, h.num_filter, &mean[0], &largest[0]); }
	if(!rc){ rc = column_shares(folded, log_2_len, h.num_filter, &mean[1], &largest[1]); }
	if(!rc){
		fprintf(stderr, "fold 2^%u -> 2^%u: set bits per column mean %.6f largest %.6f -> mean %.6f largest %.6f, false-positive rate of the largest %.6g -> %.6g, fold kernel %.3f ms\n",
		        h.log_2_filter_len, log_2_len, mean[0], largest[0], mean[1], largest[1], pow(largest[0], (double)h.num_hash), pow(largest[1], (double)h.num_hash), st.kernel_ms);
	}
	kwage_group_destroy(folded);
	kwage_group_destroy(g);
	return rc;
}

// `union` and `merge`: in.db plus one column per NEW=ACC1,ACC2[,...] -- the OR of the members' columns, made on the device in
// the group that holds them (kwage_group_union_columns) -- with the members kept (`union`) or dropped (`merge`).
static int union_db(kwage_ctx *ctx, const char *what, const char *out_db, const char *in_db, char **specs, int n, bool drop_members)
{
	// NEW=ACC1,ACC2,...: the new run accession and its members
	std::vector<std::string> names;
	std::vector<std::vector<std::string>> members(n);
	for(int i = 0; i < n; ++i){
		const std::string spec = specs[i];
		const size_t eq = spec.find('=');
		if(eq == std::string::npos || eq == 0 || eq + 1 >= spec.size()){ return usage(); }
		names.push_back(spec.substr(0, eq));
		for(size_t at = eq + 1; at <= spec.size(); ){
			const size_t comma = std::min(spec.find(',', at), spec.size());
			if(comma == at){ return usage(); }
			members[i].push_back(spec.substr(at, comma - at));
			at = comma + 1;
		}
	}
	std::vector<char*> wanted;
	for(auto &m : members){ for(std::string &a : m){ wanted.push_back(&a[0]); } }
	std::vector<std::string> have;
	int rc = read_accessions(what, in_db, wanted.data(), (int)wanted.size(), have);
	if(rc){ return rc; }
	// a member is the first column that carries the accession
	std::vector<uint64_t> columns, offsets(1, 0);
	std::vector<bool> is_member(have.size(), false);
	for(const auto &m : members){
		for(const std::string &a : m){
			const uint64_t j = (uint64_t)(std::find(have.begin(), have.end(), a) - have.begin());
			columns.push_back(j);
			is_member[j] = true;
		}
		offsets.push_back(columns.size());
	}
	kwage_db_header h;
	kwage_group *g = NULL;
	if((rc = load_db(ctx, in_db, (uint64_t)n, &h, &g))){ return rc; }
	uint64_t first = 0;
	kwage_union_stats st;
	if(kwage_group_union_columns(g, g, columns.data(), offsets.data(), (uint32_t)n, KWAGE_SEARCH_TIMING, &first, &st)){ kwage_group_destroy(g); return die(what); }
	// members keep their records; a new column gets its run accession and no other field
	std::vector<kwage_sample_info> infos(n, kwage_sample_info{});
	std::vector<kwage_save_column> cols;
	for(uint32_t j = 0; j < h.num_filter; ++j){
		if(!(drop_members && is_member[j])){ cols.push_back(kwage_save_column{j, in_db, j, NULL}); }
	}
	for(int i = 0; i < n; ++i){
		infos[i].run_accession = names[i].c_str();
		cols.push_back(kwage_save_column{first + (uint64_t)i, NULL, 0, &infos[i]});
	}
	rc = save_columns(g, out_db, cols);
	// what a union costs: the share of set bits of the new column, and the rate at which an absent k-mer passes it
	if(!rc && kwage_group_finalize(g)){ rc = die("finalize"); }
	std::vector<uint32_t> bits(kwage_group_column_span(g), 0u);
	if(!rc && kwage_group_column_bits(g, bits.data())){ rc = die("column bits"); }
	if(!rc){
		const double rows = (double)(1ull << h.log_2_filter_len);
		for(int i = 0; i < n; ++i){
			uint32_t top = 0;
			for(uint64_t c = offsets[i]; c < offsets[i + 1]; ++c){ top = std::max(top, bits[columns[c]]); }
			const double fill = (double)bits[first + (uint64_t)i]/rows;
			fprintf(stderr, "%s %s: %zu members, %u bits set of %.0f (largest member %u), fill %.6f, false-positive rate %.6g\n", what, names[i].c_str(),
			        members[i].size(), bits[first + (uint64_t)i], rows, top, fill, pow(fill, (double)h.num_hash));
		}
		fprintf(stderr, "%s: %llu entries, %llu bytes written, union kernel %.3f ms\n", what, (unsigned long long)st.entries, (unsigned long long)st.bytes_written, st.kernel_ms);
	}
	kwage_group_destroy(g);
	return rc;
}

int main(int argc, char **argv)
{
	if(argc < 3){ return usage(); }
	const std::string cmd = argv[1];

	if(cmd == "info" || cmd == "accessions"){
		kwage_db_header h;
		if(kwage_db_read_header(argv[2], &h)){ return die("read header"); }
		if(cmd == "info"){
			printf("magic\t0x%08x\nversion\t%u\ncrc32\t0x%08x\nkmer_len\t%u\nnum_hash\t%u\nlog_2_filter_len\t%u\nnum_filter\t%u\n"
			       "hash_func\t%d\ncompression\t%u\ninfo_start\t%llu\n", h.magic, h.version, h.crc32, h.kmer_len, h.num_hash,
			       h.log_2_filter_len, h.num_filter, h.hash_func, h.compression, (unsigned long long)h.info_start);
			return 0;
		}
		kwage_dbinfo *d = NULL;
		if(kwage_dbinfo_open(argv[2], &d)){ return die("read metadata"); }
		char buf[64];
		for(uint32_t j = 0; j < kwage_dbinfo_num_filter(d); ++j){
			if(kwage_dbinfo_csv_string(d, j, buf, sizeof(buf))){ kwage_dbinfo_close(d); return die("read FilterInfo"); }
			printf("%u\t%s\n", j, buf);
		}
		kwage_dbinfo_close(d);
		return 0;
	}
	if(cmd == "compress" && argc >= 4){
		return kwage_db_compress(argv[2], argv[3], argc > 4 ? (uint32_t)atoi(argv[4]) : 0) ? die("compress") : 0;
	}
	if(cmd == "decompress" && argc == 4){
		return kwage_db_decompress(argv[2], argv[3]) ? die("decompress") : 0;
	}

	// the remaining commands run on the device
	if(cmd != "build" && cmd != "repack" && cmd != "append" && cmd != "drop" && cmd != "extract" && cmd != "fold" && cmd != "union" && cmd != "merge" && cmd != "mkbloom" && cmd != "countbloom"){ return usage(); }
	kwage_ctx *ctx = NULL;
	const char *dev = getenv("KWAGE_DEVICE");
	if(kwage_init(dev ? atoi(dev) : 0, &ctx)){ return die("init"); }
	int rc = 2;
	if(cmd == "build" && argc >= 7){
		kwage_params p = {(uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[5]), (uint32_t)atoi(argv[4]), KWAGE_HASH_MURMUR32};
		kwage_build_stats st;
		rc = kwage_build_db(ctx, argv[2], &p, argv + 6, (uint32_t)(argc - 6), &st);
		if(rc){ rc = die("build"); }
		else{ fprintf(stderr, "wrote %s: %llu bytes, transpose kernel %.3f ms\n", argv[2], (unsigned long long)st.db_bytes, st.transpose_kernel_ms); }
	}
	else if(cmd == "repack" && argc >= 4){
		rc = kwage_repack_db(ctx, argv[2], argv + 3, (uint32_t)(argc - 3));
		if(rc){ rc = die("repack"); }
	}
	else if(cmd == "append" && argc >= 5){
		rc = append_blooms(ctx, argv[2], argv[3], argv + 4, (uint32_t)(argc - 4));
	}
	else if(cmd == "drop" && argc >= 5){
		rc = drop_samples(ctx, argv[2], argv[3], argv + 4, argc - 4);
	}
	else if(cmd == "extract" && argc >= 4){
		rc = extract_samples(ctx, argv[2], argv[3], argv + 4, argc - 4);
	}
	else if(cmd == "fold" && argc == 5){
		rc = fold_db(ctx, argv[2], argv[3], (uint32_t)atoi(argv[4]));
	}
	else if((cmd == "union" || cmd == "merge") && argc >= 5){
		rc = union_db(ctx, cmd.c_str(), argv[2], argv[3], argv + 4, argc - 4, cmd == "merge");
	}
	else if(cmd == "mkbloom" && argc >= 8){
		kwage_seqfile *sf = NULL;
		if(kwage_seqfile_open(argv[7], &sf)){ kwage_shutdown(ctx); return die("open sequence file"); }
		std::string concat;
		std::vector<uint64_t> off(1, 0);
		const char *d, *s;
		uint64_t n;
		int r;
		while((r = kwage_seqfile_next(sf, &d, &s, &n)) == 1){ concat.append(s, n); off.push_back(concat.size()); }
		kwage_seqfile_close(sf);
		if(r < 0){ kwage_shutdown(ctx); return die("read sequence file"); }
		kwage_params p = {(uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[6]), (uint32_t)atoi(argv[5]), KWAGE_HASH_MURMUR32};
		if(p.log_2_filter_len == 0 || p.num_hash == 0){
			kwage_batch *b = NULL;
			uint64_t distinct = 0;
			if(kwage_batch_create(ctx, concat.data(), off.data(), (uint32_t)(off.size() - 1), &b) ||
			   kwage_count_distinct_kmers(ctx, b, p.kmer_len, &distinct)){ kwage_shutdown(ctx); return die("count k-mers"); }
			kwage_batch_destroy(b);
			const float fp = argc > 8 ? (float)atof(argv[8]) : 0.25f;       // options.h:140 DEFAULT_FALSE_POSITIVE_PROBABILITY
			if(kwage_optimal_bloom_param(p.kmer_len, distinct, fp, 18, 32, &p)){ kwage_shutdown(ctx); return die("optimal_bloom_param"); }
			fprintf(stderr, "%llu distinct k-mers -> log_2_filter_len %u, num_hash %u\n", (unsigned long long)distinct, p.log_2_filter_len, p.num_hash);
		}
		kwage_sample_info si;
		memset(&si, 0, sizeof(si));
		si.run_accession = argv[3];
		si.number_of_bases = concat.size();
		rc = kwage_make_bloom(ctx, &p, concat.data(), off.data(), (uint32_t)(off.size() - 1), &si, argv[2], NULL);
		if(rc){ rc = die("mkbloom"); }
	}
	else if(cmd == "countbloom" && argc >= 7){
		float fp = 0.25f;                               // options.h:140,154-155 defaults
		uint32_t min_lg = 18, max_lg = 32;
		std::vector<const char*> files;
		for(int i = 6; i < argc; ++i){
			if(!strcmp(argv[i], "-p") && i + 1 < argc){ fp = (float)atof(argv[++i]); }
			else if(!strcmp(argv[i], "-l") && i + 1 < argc){ min_lg = (uint32_t)atoi(argv[++i]); }
			else if(!strcmp(argv[i], "-L") && i + 1 < argc){ max_lg = (uint32_t)atoi(argv[++i]); }
			else{ files.push_back(argv[i]); }
		}
		// pass 1: number of bases (the reference takes it from the SRA metadata, make_bloom.cpp:108)
		uint64_t num_bp = 0, num_reads = 0;
		const char *d, *s;
		uint64_t n;
		int r = 0;
		for(const char *f : files){
			kwage_seqfile *sf = NULL;
			if(kwage_seqfile_open(f, &sf)){ kwage_shutdown(ctx); return die("open sequence file"); }
			while((r = kwage_seqfile_next(sf, &d, &s, &n)) == 1){ num_bp += n; ++num_reads; }
			kwage_seqfile_close(sf);
			if(r < 0){ kwage_shutdown(ctx); return die("read sequence file"); }
		}
		const uint32_t logc = kwage_counting_filter_log2(num_bp);
		kwage_bloom_counter *bc = NULL;
		if(kwage_bloom_counter_create(ctx, (uint32_t)atoi(argv[4]), KWAGE_HASH_MURMUR32, (uint32_t)atoi(argv[5]), logc, max_lg, &bc)){
			kwage_shutdown(ctx); return die("countbloom");
		}
		// pass 2: fragments in file order, handed over in batches of ~64 MB
		std::string concat;
		std::vector<uint64_t> off(1, 0);
		rc = 0;
		for(size_t fi = 0; fi < files.size() && !rc; ++fi){
			kwage_seqfile *sf = NULL;
			if(kwage_seqfile_open(files[fi], &sf)){ rc = die("open sequence file"); break; }
			while(!rc && (r = kwage_seqfile_next(sf, &d, &s, &n)) == 1){
				concat.append(s, n); off.push_back(concat.size());
				if(concat.size() >= (64u << 20)){
					if(kwage_bloom_counter_add(bc, concat.data(), off.data(), (uint32_t)(off.size() - 1))){ rc = die("countbloom"); }
					concat.clear(); off.assign(1, 0);
				}
			}
			kwage_seqfile_close(sf);
			if(!rc && r < 0){ rc = die("read sequence file"); }
		}
		if(!rc && off.size() > 1 && kwage_bloom_counter_add(bc, concat.data(), off.data(), (uint32_t)(off.size() - 1))){ rc = die("countbloom"); }
		if(!rc){
			kwage_sample_info si;
			memset(&si, 0, sizeof(si));
			si.run_accession = argv[3];
			si.number_of_spots = num_reads;
			si.number_of_bases = num_bp;
			kwage_params p;
			int status = KWAGE_BLOOM_INVALID;
			kwage_bloom_counter_stats st;
			if(kwage_bloom_counter_get_stats(bc, &st) || kwage_bloom_counter_finish(bc, fp, min_lg, &si, argv[2], &p, &status)){ rc = die("countbloom"); }
			else if(status != KWAGE_BLOOM_SUCCESS){
				fprintf(stderr, "%llu bases, %llu k-mers with count >= %s: no Bloom parameters satisfy the bound (STATUS_BLOOM_INVALID)\n",
				        (unsigned long long)st.num_bp, (unsigned long long)st.num_valid_kmer, argv[5]);
				rc = 3;
			}
			else{
				fprintf(stderr, "%llu bases, counting filters 2^%u, %llu k-mers with count >= %s -> log_2_filter_len %u, num_hash %u\n",
				        (unsigned long long)st.num_bp, logc, (unsigned long long)st.num_valid_kmer, argv[5], p.log_2_filter_len, p.num_hash);
			}
		}
		kwage_bloom_counter_destroy(bc);
	}
	else{
		rc = usage();
	}
	kwage_shutdown(ctx);
	return rc;
}
