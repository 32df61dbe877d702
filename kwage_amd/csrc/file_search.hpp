// kwage_amd/csrc/file_search.hpp -- what the programs share that search the database file by file, one group per file, so
// that it never has to fit the device at once (kwage_top, kwage_scores, kwage_presence, kwage_near): the owners of the
// device context, of one file's group and of the query batches' device copies, the loop "every file against every batch",
// and what the two matrix programs print alike.  Included after cli_common.hpp.
//
// Whatever ends a run, the group goes first, then the batches' device copies (in kwage_near the filter sets), then the
// context: declare a Device before what lives on it, and C++ destroys them in that order.
//
// Environment: KWAGE_DEVICE (HIP device index, default 0), KWAGE_BATCH_BASES (bases per query batch, default 64 Mi).
#ifndef KWAGE_AMD_FILE_SEARCH_HPP
#define KWAGE_AMD_FILE_SEARCH_HPP

#include "cli_common.hpp"

namespace {

// The run's device context, shut down with this object.
struct Device {
	kwage_ctx *ctx = nullptr;
	Device()
	{
		check(kwage_init((int)env_u64("KWAGE_DEVICE", 0), &ctx));
		one_shot_placement(ctx);
	}
	~Device() { kwage_shutdown(ctx); }
	Device(const Device&) = delete;
	Device &operator=(const Device&) = delete;
};

// One file as a finalized group of its own, destroyed with this object.
struct FileGroup {
	unique_ptr<kwage_group, void (*)(kwage_group*)> group{nullptr, kwage_group_destroy};
	uint64_t first = 0;                 // the file's first column in the group
	uint32_t nf = 0;                    // and how many it has
	FileGroup(kwage_ctx *ctx, const DbFileEntry &f)
	{
		const kwage_db_header &h = f.header;
		kwage_params p{h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func};
		kwage_group *g = nullptr;
		check(kwage_group_create(ctx, &p, h.num_filter, &g));
		group.reset(g);                 // (owned from here on, also when the constructor throws)
		check(kwage_group_add_db_file(g, f.path.c_str(), &first, &nf));
		check(kwage_group_finalize(g));
	}
	kwage_group *get() const { return group.get(); }
};

// A batch of queries, its copy on the device, and what the program keeps per batch (its block of a matrix, say).
template<class Payload> struct ResidentBatch {
	QueryBatch q;
	kwage_batch *b = nullptr;
	bool typed = false;                 // from the command line
	Payload kept;
};

// Every query, in batches, in kwage's order: the sequences of the command line, then the records of the -i files (the
// query set stays in host and device memory for the whole run).  `prepare` gives each batch what it keeps; when it
// returns false the reading ends, and so does this.
template<class Payload, class Prepare> bool read_queries(const Cli &cli, deque<ResidentBatch<Payload> > &batches, Prepare prepare)
{
	const uint64_t max_bases = env_u64("KWAGE_BATCH_BASES", 64ull << 20);
	CommandLineQueries typed(cli.query_seqs);
	FileQueries from_disk(cli.query_files);
	for(QuerySource *src : {(QuerySource*)&typed, (QuerySource*)&from_disk}){
		for(;;){
			ResidentBatch<Payload> rb;
			if(!src->fill(rb.q, max_bases)){ break; }
			rb.typed = (src == &typed);
			if(!prepare(rb)){ return false; }
			batches.push_back(std::move(rb));
		}
	}
	return true;
}

// The batches' copies on the device, destroyed with this object.
template<class Payload> struct DeviceCopies {
	deque<ResidentBatch<Payload> > &batches;
	explicit DeviceCopies(deque<ResidentBatch<Payload> > &all) : batches(all) {}
	void make(kwage_ctx *ctx)
	{
		for(ResidentBatch<Payload> &rb : batches){
			check(kwage_batch_create(ctx, rb.q.bases.data(), rb.q.offsets.data(), (uint32_t)rb.q.size(), &rb.b));
		}
	}
	~DeviceCopies()
	{
		for(ResidentBatch<Payload> &rb : batches){
			if(rb.b){ kwage_batch_destroy(rb.b); rb.b = nullptr; }
		}
	}
};

// The search: a device, every batch on it, then file by file -- the file's group, and each(index of the file, its
// group, the batch) for every batch.  The device is shut down when this returns; what `each` kept is the caller's.
template<class Payload, class Each> void search_file_by_file(const vector<DbFileEntry> &files, deque<ResidentBatch<Payload> > &batches, Each each)
{
	Device device;                              // (declared first: shut down last)
	DeviceCopies<Payload> copies(batches);
	copies.make(device.ctx);
	for(size_t fi = 0; fi < files.size(); ++fi){
		const FileGroup g(device.ctx, files[fi]);
		for(ResidentBatch<Payload> &rb : batches){ each(fi, g, rb); }
	}
}

// =====================================================================================================
// a matrix, queries x samples (kwage_scores, kwage_presence)
// =====================================================================================================
// Samples come in database order (files as found, columns within a file): every file's first sample in the matrix goes to
// its first_column.  Returns the number of samples.
uint64_t place_samples(vector<DbFileEntry> &files)
{
	uint64_t samples = 0;
	for(DbFileEntry &f : files){
		f.first_column = samples;
		samples += f.header.num_filter;
	}
	return samples;
}

// A batch's block of the matrix, `n` zeroed cells.  False: it does not fit (said on stderr; `row_size` names a row's).
template<class Cells> bool zeroed_block(Cells &cells, uint64_t n, uint64_t samples, const char *row_size)
{
	try{ cells.assign(n, 0); }
	catch(const std::bad_alloc&){
		cerr << "The matrix does not fit in host memory: " << samples << " samples " << row_size << " for every query" << endl;
		return false;
	}
	return true;
}

// The header line: `leading` (the columns before the samples), then one run accession per sample.
void put_matrix_header(TextSink &to, const char *leading, const vector<DbFileEntry> &files, const vector<DbInfo> &infos)
{
	to.put(leading);
	for(size_t fi = 0; fi < files.size(); ++fi){
		for(uint32_t c = 0; c < files[fi].header.num_filter; ++c){
			FilterInfo info;
			if(!infos[fi].info(c, info)){ throw "binary_read<FilterInfo>: Unable to read FilterInfo"; }
			to.put('\t'); to.put(info.csv_string());
			to.drain();
		}
	}
	to.put('\n');
}

// A line's first cell: the query's name as kwage reports it.
template<class Payload> void put_query_name(TextSink &to, const ResidentBatch<Payload> &rb, size_t q)
{
	if(rb.typed){ to.put("command line seq "); to.put((uint64_t)rb.q.ids[q]); }
	else{ to.put(rb.q.deflines[q]); }
}

}  // namespace

#endif
