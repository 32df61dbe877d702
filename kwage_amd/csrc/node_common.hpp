// kwage_amd/csrc/node_common.hpp -- what the one-process-per-GPU programs share (kwage_node, kwage_top_node): the plan
// (database files grouped by parameters, every group's files dealt to the ranks, global column numbers, passes), the
// bootstrap and set-up of the RCCL communicator with its timeout, the rehearsal segment (KWAGE_NODE_REHEARSE), the
// exchange's building blocks (count all-gather, grouped send / recv to rank 0) and the fork / wait / kill loop of the
// ranks.  kwage_node.cpp's header comment describes the scheme and the environment.  Included after cli_common.hpp.
#ifndef KWAGE_AMD_NODE_COMMON_HPP
#define KWAGE_AMD_NODE_COMMON_HPP

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <pthread.h>
#include <sys/mman.h>
#include <functional>
#include <new>

#include "cli_common.hpp"

namespace {

#define NODE_HIP(call) do { hipError_t e_ = (call); if(e_ != hipSuccess){ throw string(#call " failed: ") + hipGetErrorString(e_); } } while(0)
#define NODE_NCCL(call) do { ncclResult_t r_ = (call); if(r_ != ncclSuccess){ throw string(#call " failed: ") + ncclGetErrorString(r_); } } while(0)

struct GroupKey {
	uint32_t kmer_len, num_hash, log_2_filter_len; int32_t hash_func;
	bool operator<(const GroupKey &o) const
	{
		return std::tie(kmer_len, num_hash, log_2_filter_len, hash_func) < std::tie(o.kmer_len, o.num_hash, o.log_2_filter_len, o.hash_func);
	}
};

// One rank's share of one group: its files and where each file's columns begin in the rank's matrix.  Every rank can
// compute every rank's share -- and its layout -- from the headers alone.
struct Share {
	vector<uint32_t> files;              // indices into the list of database files
	vector<uint64_t> first_column;       // of each file's block (blocks start at 16-byte boundaries)
	uint64_t span_columns = 0;           // next free column
};

Share share_of(const vector<uint32_t> &group_files, const vector<DbFileEntry> &files, size_t rank, size_t n_ranks)
{
	uint64_t total = 0, before = 0, span = 0;
	for(uint32_t fi : group_files){ total += files[fi].header.num_filter; }
	Share s;
	for(uint32_t fi : group_files){
		const uint64_t nf = files[fi].header.num_filter;
		const size_t owner = min<size_t>(n_ranks - 1, (size_t)(((long double)before + nf/2.0L)*n_ranks/max<uint64_t>(total, 1)));
		if(owner == rank){
			span = (span + 15)/16*16;
			s.files.push_back(fi);
			s.first_column.push_back(span*8);
			span += (nf + 7)/8;
		}
		before += nf;
	}
	s.span_columns = span*8;
	return s;
}

// What one rank holds resident in one pass: a span of whole files of one group, one matrix.  The records it produces carry
// base + column-in-matrix, which is the file's place in the GLOBAL numbering whatever the pass (a unit starts at a file,
// and files follow each other in a unit exactly as in the rank's whole share: blocks at 16-byte boundaries).
struct Unit {
	size_t gi = 0;                       // index into the groups
	vector<uint32_t> files;              // indices into the list of database files
	vector<uint64_t> first_column;       // of each file's block within the unit's matrix
	uint64_t span_columns = 0;
	uint64_t base = 0;                   // global number of the unit's column 0
	uint32_t kmer_len = 0;
	kwage_group *mine = nullptr;
};

// A file's columns in the global numbering of the hit records.
struct ColumnBlock { uint64_t first_global_column; uint32_t file_index, kmer_len; };

struct NodeGroup {
	GroupKey key;
	kwage_params params;
	vector<Share> share;                 // per rank
	vector<uint64_t> base;               // per rank: global number of the rank's column 0 of this group
};

// How rank 0 hands the communicator's unique id to the other ranks: anonymous shared memory mapped before the fork.
struct Bootstrap {
	ncclUniqueId id;
	volatile int ready = 0;
};

double now_seconds() { return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count(); }

// KWAGE_NODE_REHEARSE: what the ranks share instead of a communicator (mapped before the fork)
struct Rehearsal {
	pthread_barrier_t barrier;
	uint64_t capacity;                   // records
	uint64_t counts[64];
	kwage_hit *records() { return reinterpret_cast<kwage_hit*>(this + 1); }
};

// The node's plan: the database files grouped by parameters, every group's files dealt to the ranks (share_of), and
// the global column number of every rank's column 0 -- group after group, inside a group rank after rank.  A pure
// function of the file headers: every rank computes the same plan (and KWAGE_NODE_PLAN=1 prints it without a device).
vector<NodeGroup> plan_groups(const vector<DbFileEntry> &files, int n_ranks)
{
	map<GroupKey, vector<uint32_t> > by_key;
	for(size_t i = 0; i < files.size(); ++i){
		const kwage_db_header &h = files[i].header;
		by_key[GroupKey{h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func}].push_back((uint32_t)i);
	}
	vector<NodeGroup> groups;
	uint64_t next_base = 0;
	for(const auto &kv : by_key){
		NodeGroup g;
		g.key = kv.first;
		g.params = kwage_params{kv.first.kmer_len, kv.first.num_hash, kv.first.log_2_filter_len, kv.first.hash_func};
		for(int r = 0; r < n_ranks; ++r){
			g.share.push_back(share_of(kv.second, files, (size_t)r, (size_t)n_ranks));
			g.base.push_back(next_base);
			next_base += g.share.back().span_columns;
		}
		groups.push_back(std::move(g));
	}
	if(next_base > (1ull << 32)){ throw "main: more than 2^32 columns in the database"; }
	return groups;
}

// The passes of one rank (kwage_main.cpp's packing): its files of every group, in order, cut into units that fit what is
// left of `budget` bytes in the current pass; a file that does not fit goes to the next pass -- unless the pass is still
// empty: then it is tried alone (and the allocation reports it if it really is too large).
vector<vector<Unit> > plan_passes(const vector<NodeGroup> &groups, const vector<DbFileEntry> &files, size_t rank, uint64_t budget)
{
	vector<vector<Unit> > passes(1);
	uint64_t pass_left = budget;
	for(size_t gi = 0; gi < groups.size(); ++gi){
		const Share &sh = groups[gi].share[rank];
		const uint64_t nrows = 1ull << groups[gi].params.log_2_filter_len;
		for(size_t m0 = 0; m0 < sh.files.size(); ){
			uint64_t span_bytes = 0;
			size_t m1 = m0;
			Unit u;
			while(m1 < sh.files.size()){
				const uint64_t at = (span_bytes + 15)/16*16;
				const uint64_t next = at + ((uint64_t)files[sh.files[m1]].header.num_filter + 7)/8;
				if(((next + 127)/128*128)*nrows > pass_left && (m1 > m0 || !passes.back().empty())){ break; }
				u.files.push_back(sh.files[m1]);
				u.first_column.push_back(at*8);
				span_bytes = next;
				++m1;
			}
			if(m1 > m0){
				u.gi = gi;
				u.span_columns = span_bytes*8;
				u.base = groups[gi].base[rank] + sh.first_column[m0];
				u.kmer_len = groups[gi].params.kmer_len;
				pass_left -= min(pass_left, ((span_bytes + 127)/128*128)*nrows);
				passes.back().push_back(std::move(u));
				m0 = m1;
			}
			if(m0 < sh.files.size()){ passes.emplace_back(); pass_left = budget; }
		}
	}
	if(passes.back().empty() && passes.size() > 1){ passes.pop_back(); }
	return passes;
}

// KWAGE_NODE_PLAN=1: print the plan for n_ranks ranks and stop -- no device is touched (tests; a dry run before a long job)
int print_plan(const vector<string> &db_paths, int n_ranks)
{
	return guarded([&]() -> int {
		vector<DbFileEntry> files;
		read_database_files(db_paths, files, nullptr);
		const vector<NodeGroup> groups = plan_groups(files, n_ranks);
		cout << "{\"ranks\": " << n_ranks << ", \"groups\": [";
		for(size_t gi = 0; gi < groups.size(); ++gi){
			const NodeGroup &g = groups[gi];
			cout << (gi ? ", " : "") << "{\"kmer_len\": " << g.key.kmer_len << ", \"num_hash\": " << g.key.num_hash << ", \"log_2_filter_len\": "
			     << g.key.log_2_filter_len << ", \"hash_func\": " << g.key.hash_func << ", \"shares\": [";
			for(size_t r = 0; r < g.share.size(); ++r){
				cout << (r ? ", " : "") << "{\"rank\": " << r << ", \"global_base\": " << g.base[r] << ", \"span_columns\": " << g.share[r].span_columns << ", \"files\": [";
				for(size_t f = 0; f < g.share[r].files.size(); ++f){
					cout << (f ? ", " : "") << "{\"path\": \"" << files[g.share[r].files[f]].path << "\", \"first_column\": " << g.share[r].first_column[f]
					     << ", \"num_filter\": " << files[g.share[r].files[f]].header.num_filter << "}";
				}
				cout << "]}";
			}
			cout << "]}";
		}
		cout << "]";
		// with a budget (KWAGE_MAX_GROUP_BYTES): every rank's passes as plan_passes cuts them, the ranks padded to the same number
		const uint64_t budget = env_u64("KWAGE_MAX_GROUP_BYTES", 0);
		if(budget){
			size_t n_passes = 1;
			vector<vector<vector<Unit> > > per_rank((size_t)n_ranks);
			for(int r = 0; r < n_ranks; ++r){
				per_rank[(size_t)r] = plan_passes(groups, files, (size_t)r, budget);
				n_passes = max(n_passes, per_rank[(size_t)r].size());
			}
			cout << ", \"budget\": " << budget << ", \"passes\": " << n_passes << ", \"rank_passes\": [";
			for(int r = 0; r < n_ranks; ++r){
				per_rank[(size_t)r].resize(n_passes);
				cout << (r ? ", " : "") << "[";
				for(size_t ps = 0; ps < n_passes; ++ps){
					cout << (ps ? ", " : "") << "[";
					for(size_t ui = 0; ui < per_rank[(size_t)r][ps].size(); ++ui){
						const Unit &u = per_rank[(size_t)r][ps][ui];
						cout << (ui ? ", " : "") << "{\"group\": " << u.gi << ", \"global_base\": " << u.base << ", \"span_columns\": " << u.span_columns << ", \"files\": [";
						for(size_t f = 0; f < u.files.size(); ++f){
							cout << (f ? ", " : "") << "{\"path\": \"" << files[u.files[f]].path << "\", \"first_column\": " << u.first_column[f] << "}";
						}
						cout << "]}";
					}
					cout << "]";
				}
				cout << "]";
			}
			cout << "]";
		}
		cout << "}" << endl;
		return EXIT_SUCCESS;
	});
}

// The RCCL communicator of `rank` (not for a rehearsal): rank 0 makes the unique id and leaves it in `boot`, every rank
// brings the communicator up on a thread of its own under KWAGE_NODE_COMM_TIMEOUT_S.
ncclComm_t node_comm_init(int rank, int n_ranks, Bootstrap *boot)
{
	ncclComm_t comm = nullptr;
	// stdout is the report: whatever RCCL prints while a communicator comes up (its version banner under
	// NCCL_DEBUG=VERSION goes to stdout whatever NCCL_DEBUG_FILE says) is sent to stderr instead
	cout.flush(); fflush(stdout);
	const int report_fd = dup(STDOUT_FILENO);
	if(report_fd < 0 || dup2(STDERR_FILENO, STDOUT_FILENO) < 0){ throw string("cannot redirect stdout"); }
	// the communicator's id travels through memory the ranks have shared since before the fork: nothing another
	// user of the machine could plant or read (round 3 used a file under /tmp)
	ncclUniqueId id;
	if(rank == 0){
		NODE_NCCL(ncclGetUniqueId(&id));
		memcpy(&boot->id, &id, sizeof(id));
		__sync_synchronize();
		boot->ready = 1;
	}
	else{
		int tries = 0;
		while(!boot->ready && tries++ < 60000){ usleep(1000); }
		if(!boot->ready){ throw string("no RCCL unique id from rank 0"); }
		__sync_synchronize();
		memcpy(&id, &boot->id, sizeof(id));
	}
	// ncclCommInitRank has no timeout of its own: a rank whose peers never arrive (one of them failed before this point)
	// would wait forever.  It runs on a thread; if it is not back in time the process exits non-zero without
	// returning into RCCL, and the parent ends the other ranks.
	ncclResult_t comm_up = ncclInternalError;
	{
		struct Up { mutex mu; condition_variable cv; bool done = false; ncclResult_t rc = ncclInternalError; ncclComm_t comm = nullptr; };
		shared_ptr<Up> up = make_shared<Up>();
		const int device = rank;
		thread([up, n_ranks, id, rank, device]() {
			(void)hipSetDevice(device);
			ncclComm_t c = nullptr;
			const ncclResult_t rc = ncclCommInitRank(&c, n_ranks, id, rank);
			lock_guard<mutex> lk(up->mu);
			up->rc = rc; up->comm = c; up->done = true;
			up->cv.notify_all();
		}).detach();
		unique_lock<mutex> lk(up->mu);
		const uint64_t limit_s = env_u64("KWAGE_NODE_COMM_TIMEOUT_S", 120);
		if(!up->cv.wait_for(lk, chrono::seconds(limit_s), [&]{ return up->done; })){
			cerr << "Caught the error rank " << rank << ": the RCCL communicator did not come up within " << limit_s << " s (a peer is missing)" << endl;
			fflush(nullptr);
			_exit(EXIT_FAILURE);
		}
		comm_up = up->rc;
		comm = up->comm;
	}
	fflush(stdout);
	dup2(report_fd, STDOUT_FILENO);
	close(report_fd);
	if(comm_up != ncclSuccess){ throw string("ncclCommInitRank failed: ") + ncclGetErrorString(comm_up); }
	return comm;
}

// Every rank's budget to everyone (KWAGE_MAX_GROUP_BYTES, or what is free on the device), then every rank plans every
// rank's passes: all of them make the same number of exchanges.  Returns this rank's passes, padded to *n_passes.
vector<vector<Unit> > node_plan_rank_passes(const char *program, kwage_ctx *ctx, int rank, int n_ranks, const vector<NodeGroup> &groups,
                                            const vector<DbFileEntry> &files, Rehearsal *rehearsal, ncclComm_t comm, hipStream_t stream,
                                            uint64_t *d_counts, uint64_t *h_counts, bool stats, size_t *n_passes_out)
{
	vector<vector<Unit> > my_passes;
	size_t n_passes = 1;
	uint64_t budget = env_u64("KWAGE_MAX_GROUP_BYTES", 0);
	if(budget == 0){
		uint64_t free_b = 0, total_b = 0;
		check(kwage_mem_info(ctx, &free_b, &total_b));
		budget = free_b - free_b/8;              // leave room for staging buffers, row indices, hits
		if(rehearsal){ budget /= (uint64_t)n_ranks; }      // (the rehearsed ranks share one device)
	}
	vector<uint64_t> budgets((size_t)n_ranks, budget);
	if(rehearsal){
		rehearsal->counts[rank] = budget;
		pthread_barrier_wait(&rehearsal->barrier);
		for(int r = 0; r < n_ranks; ++r){ budgets[(size_t)r] = rehearsal->counts[r]; }
		pthread_barrier_wait(&rehearsal->barrier);
	}
	else if(n_ranks > 1){
		uint64_t *d_mine = nullptr;
		NODE_HIP(hipMalloc((void**)&d_mine, sizeof(uint64_t)));
		NODE_HIP(hipMemcpy(d_mine, &budget, sizeof(uint64_t), hipMemcpyHostToDevice));
		NODE_NCCL(ncclAllGather(d_mine, d_counts, 1, ncclUint64, comm, stream));
		NODE_HIP(hipMemcpyAsync(h_counts, d_counts, (size_t)n_ranks*sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
		NODE_HIP(hipStreamSynchronize(stream));
		for(int r = 0; r < n_ranks; ++r){ budgets[(size_t)r] = h_counts[r]; }
		(void)hipFree(d_mine);
	}
	for(int r = 0; r < n_ranks; ++r){
		vector<vector<Unit> > pr = plan_passes(groups, files, (size_t)r, budgets[(size_t)r]);
		n_passes = max(n_passes, pr.size());
		if(r == rank){ my_passes = std::move(pr); }
	}
	my_passes.resize(n_passes);
	if(env_u64("KWAGE_VERBOSE", 0) || stats){
		size_t nu = 0;
		for(const auto &ps : my_passes){ nu += ps.size(); }
		// (one write: the ranks share stderr)
		fprintf(stderr, "[%s] rank %d: budget %llu bytes per pass, %zu pass(es), %zu unit(s) of its own\n", program, rank, (unsigned long long)budget, n_passes, nu);
	}
	*n_passes_out = n_passes;
	return my_passes;
}

// The count all-gather of an exchange, straight from a list's device counter word; h_counts holds every rank's count once
// `stream` has been waited for.
void node_counts_start(const uint64_t *d_count, uint64_t *d_counts, uint64_t *h_counts, int n_ranks, ncclComm_t comm, hipStream_t stream)
{
	NODE_NCCL(ncclAllGather(d_count, d_counts, 1, ncclUint64, comm, stream));
	NODE_HIP(hipMemcpyAsync(h_counts, d_counts, (size_t)n_ranks*sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
}

// The records of an exchange in exact sizes to rank 0 (one grouped ncclSend / ncclRecv; RCCL has no gatherv): rank r's
// go to d_all + counts[0] + ... + counts[r-1] on rank 0; rank 0's own are not moved.
void node_send_recv(int rank, int n_ranks, const vector<uint64_t> &counts, const kwage_hit *d_hits, uint64_t n_mine, kwage_hit *d_all,
                    ncclComm_t comm, hipStream_t stream)
{
	NODE_NCCL(ncclGroupStart());
	if(rank == 0){
		uint64_t at = counts[0];
		for(int r = 1; r < n_ranks; ++r){
			if(counts[(size_t)r]){ NODE_NCCL(ncclRecv(d_all + at, counts[(size_t)r]*3, ncclUint32, r, comm, stream)); }
			at += counts[(size_t)r];
		}
	}
	else if(n_mine){
		NODE_NCCL(ncclSend(d_hits, n_mine*3, ncclUint32, 0, comm, stream));
	}
	NODE_NCCL(ncclGroupEnd());
}

// KWAGE_NODE_REHEARSE: the counts of an exchange and every rank's records into the shared segment (rank after rank).
// Afterwards rank 0 reads the segment; the caller then waits at the barrier once more (the segment is free again).
void rehearse_gather(Rehearsal *rehearsal, int rank, int n_ranks, const kwage_hit *d_hits, uint64_t n_mine, vector<uint64_t> &counts, uint64_t &total)
{
	rehearsal->counts[rank] = n_mine;
	pthread_barrier_wait(&rehearsal->barrier);
	uint64_t at = 0;
	for(int r = 0; r < n_ranks; ++r){
		counts[(size_t)r] = rehearsal->counts[r];
		if(r < rank){ at += counts[(size_t)r]; }
		total += counts[(size_t)r];
	}
	if(total > rehearsal->capacity){ throw string("the rehearsal segment is too small for this hit list"); }
	if(n_mine){ NODE_HIP(hipMemcpy(rehearsal->records() + at, d_hits, n_mine*sizeof(kwage_hit), hipMemcpyDeviceToHost)); }
	pthread_barrier_wait(&rehearsal->barrier);
}

// A program's main after its options are read: the plan (KWAGE_NODE_PLAN), the rank count, the rehearsal segment, the
// bootstrap, and the ranks forked before anything touches a device -- `run_rank` runs in each; a rank that fails ends
// the others.
int node_main(const char *program, const vector<string> &db_paths,
              const function<int(int rank, int n_ranks, Bootstrap *boot, Rehearsal *rehearsal)> &run_rank)
{
	int n_ranks = (int)env_u64("KWAGE_NODE_RANKS", 0);
	// the plan is a function of the file headers and the rank count: it is printed before anything looks for a device
	if(env_u64("KWAGE_NODE_PLAN", 0)){
		if(n_ranks < 1 || n_ranks > 64){
			cerr << program << ": KWAGE_NODE_PLAN needs the number of ranks in KWAGE_NODE_RANKS (1..64); no device is asked" << endl;
			return EXIT_FAILURE;
		}
		return print_plan(db_paths, n_ranks);
	}
	// the parent touches no GPU: the devices are counted by a short-lived child, the ranks forked before any HIP call
	if(n_ranks <= 0){ n_ranks = device_count_in_child(); }
	if(n_ranks < 1 || n_ranks > 64){
		cerr << program << ": no usable device count (" << n_ranks << "); set KWAGE_NODE_RANKS" << endl;
		return EXIT_FAILURE;
	}
	Rehearsal *rehearsal = nullptr;
	if(env_u64("KWAGE_NODE_REHEARSE", 0)){
		const uint64_t capacity = env_u64("KWAGE_NODE_REHEARSE_RECORDS", 64ull << 20);
		void *seg = mmap(nullptr, sizeof(Rehearsal) + capacity*sizeof(kwage_hit), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
		if(seg == MAP_FAILED){ perror("mmap"); return EXIT_FAILURE; }
		rehearsal = static_cast<Rehearsal*>(seg);
		rehearsal->capacity = capacity;
		pthread_barrierattr_t shared;
		pthread_barrierattr_init(&shared);
		pthread_barrierattr_setpshared(&shared, PTHREAD_PROCESS_SHARED);
		pthread_barrier_init(&rehearsal->barrier, &shared, (unsigned)n_ranks);
	}
	// where rank 0 leaves the communicator's id for the others: anonymous memory shared with the ranks through the fork
	void *bseg = mmap(nullptr, sizeof(Bootstrap), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
	if(bseg == MAP_FAILED){ perror("mmap"); return EXIT_FAILURE; }
	Bootstrap *boot = new (bseg) Bootstrap();
	vector<pid_t> kids;
	int rc = EXIT_SUCCESS;
	for(int r = 0; r < n_ranks; ++r){
		const pid_t pid = fork();
		if(pid < 0){
			// the ranks already started would wait for this one in the communicator's set-up or the first exchange: end them
			perror("fork");
			rc = EXIT_FAILURE;
			for(pid_t k : kids){ kill(k, SIGTERM); }
			break;
		}
		if(pid == 0){
			const int rank_rc = run_rank(r, n_ranks, boot, rehearsal);
			cout.flush();
			fflush(nullptr);
			_exit(rank_rc);
		}
		kids.push_back(pid);
	}
	// a rank that fails would leave the others waiting in the exchange: end them too
	for(size_t left = kids.size(); left; ){
		int st = 0;
		const pid_t done = waitpid(-1, &st, 0);
		if(done < 0){ break; }
		vector<pid_t>::iterator it = find(kids.begin(), kids.end(), done);
		if(it == kids.end()){ continue; }
		*it = 0;
		--left;
		if((!WIFEXITED(st) || WEXITSTATUS(st) != 0) && rc == EXIT_SUCCESS){
			rc = EXIT_FAILURE;
			for(pid_t k : kids){ if(k > 0){ kill(k, SIGTERM); } }
		}
	}
	(void)munmap(bseg, sizeof(Bootstrap));
	return rc;
}

}  // namespace

#endif
