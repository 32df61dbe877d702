// tests/sanitize/search_plan_sanitize.cpp -- the host-side plan of the threshold search's gather stage
// (kwage_amd/csrc/search_plan.hpp) under -fsanitize=address,undefined.  No device: the program reads a text file of cases,
// plans each one twice (the two plans must agree in every field printed), checks the truncated walk's tables where they
// are filled -- in allocations of exactly their size -- and prints a line per case for tests/test_search_plan.py.
//   search_plan_sanitize CASES.txt
// A case is one line of numbers:
//   id ncu stride nrows num_hash alloc_bytes mixes_regions density_max threshold flags blocks_per_cu
//   nknobs (name value) x nknobs  ngroups (count npos) x ngroups
// -- the batch's queries as runs of `count` queries of `npos` k-mer positions each.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "search_plan.hpp"

using namespace kwage;

// host.cpp's kwage_make_bloom calls into the device library, which is not linked here (and never called)
extern "C" int kwage_batch_create(kwage_ctx*, const char*, const uint64_t*, uint32_t, kwage_batch**) { return -1; }
extern "C" void kwage_batch_destroy(kwage_batch*) {}
extern "C" int kwage_bloom_bits_from_batch(kwage_ctx*, const kwage_params*, kwage_batch*, void*, uint64_t*) { return -1; }

static long checks = 0, refused = 0, tables = 0;
#define EXPECT(c) do { ++checks; if(!(c)){ fprintf(stderr, "FAILED %s:%d: %s (case %ld)\n", __FILE__, __LINE__, #c, id); return 1; } } while(0)

// the knobs the plan reads, by the names kwage_ctx_set_tuning knows them under
struct Knob { const char *name; int64_t Tuning::*field; };
static const Knob KNOBS[] = {
	{"walk", &Tuning::walk}, {"walk_min_rows", &Tuning::walk_min_rows}, {"walk_max_kib", &Tuning::walk_max_kib}, {"walk_tile_kib", &Tuning::walk_tile_kib},
	{"walk_min_kib", &Tuning::walk_min_kib}, {"walk_waves", &Tuning::walk_waves}, {"walk_one_wg_per_cu", &Tuning::walk_one_wg_per_cu},
	{"walk_bands", &Tuning::walk_bands}, {"walk_bands_min_gib", &Tuning::walk_bands_min_gib}, {"and_vec", &Tuning::and_vec},
	{"and_wide_min_kib", &Tuning::and_wide_min_kib}, {"and_wide", &Tuning::and_wide}, {"narrow", &Tuning::narrow}, {"force_segs", &Tuning::force_segs},
	{"ee_refine", &Tuning::ee_refine}, {"refine_seg_rows", &Tuning::refine_seg_rows}, {"refine_min_rows", &Tuning::refine_min_rows},
	{"refine_max_groups", &Tuning::refine_max_groups}, {"refine_unroll", &Tuning::refine_unroll}, {"screen_wpc", &Tuning::screen_wpc},
	{"count_screen_wpc", &Tuning::count_screen_wpc}, {"count_screen_min_tiles", &Tuning::count_screen_min_tiles}, {"count_trunc", &Tuning::count_trunc},
	{"count_screen_check", &Tuning::count_screen_check}, {"refine_static", &Tuning::refine_static}, {"refine_list_cap", &Tuning::refine_list_cap},
	{"count_walk", &Tuning::count_walk}, {"count_walk_wpc", &Tuning::count_walk_wpc}, {"count_walk_waves", &Tuning::count_walk_waves},
	{"count_walk_min_rows", &Tuning::count_walk_min_rows},
};

static uint32_t blocks_per_cu = 2;
static uint32_t screen_blocks(uint32_t, uint32_t) { return blocks_per_cu; }

// every field a launch depends on, as one line
static std::string show(int rc, const SearchPlan &p)
{
	char name[64] = "-", buf[1024];
	if(rc == KWAGE_OK){ format_search_name(p, name, sizeof(name)); }
	const RefinePlan &r = p.refine;
	snprintf(buf, sizeof(buf), "rc=%d name=%s form=%d vec=%d unroll=%d up=%d ch=%u G=%u planes=%u seg_planes=%u tplanes=%u nh=%u segs=%u seg_kmers=%u chunks=%u "
	         "wgs=%u wg_waves=%u lds=%zu combine_wgs=%u finish_wgs=%u bands=%u rows_per_band=%u total_slots=%" PRIu64 " per_wave=%" PRIu64 " "
	         "refine_wgs=%u emit_wgs=%u seg_rows=%u clusters=%" PRIu64 " items=%" PRIu64 " units=%" PRIu64 " lc=%u/%u/%u/%u li=%u/%u/%u/%u lu=%u/%u/%u/%u "
	         "partial_bytes=%" PRIu64 " exchange_bytes=%" PRIu64 " flags_bytes=%" PRIu64 " band_rows_bytes=%" PRIu64 " band_loc_bytes=%" PRIu64 " trunc_bytes=%" PRIu64 " seg=%" PRIu64,
	         rc, name, (int)p.form, p.vec, p.unroll, p.up, p.ch, p.G, p.planes, p.seg_planes, p.tplanes, p.nh, p.segs, p.seg_kmers, p.chunks,
	         p.wgs, p.wg_waves, p.lds, p.combine_wgs, p.finish_wgs, p.bands, p.rows_per_band, p.total_slots, p.per_wave,
	         r.refine_wgs, r.emit_wgs, r.seg_rows, r.clusters, r.items, r.units, r.lc.cap, r.lc.stat, r.lc.base, r.lc.chunk, r.li.cap, r.li.stat, r.li.base, r.li.chunk,
	         r.lu.cap, r.lu.stat, r.lu.base, r.lu.chunk,
	         p.partial_bytes, p.exchange_bytes, p.flags_bytes, p.band_rows_bytes, p.band_loc_bytes, p.trunc_bytes, p.seg);
	return buf;
}

static int run_case(FILE *f, long id)
{
	Tuning tn;
	SearchInputs in;
	unsigned long long ncu, stride, nrows, alloc;
	unsigned num_hash, mixes, flags, bpc, nknobs, ngroups;
	double density_max, threshold;
	EXPECT(fscanf(f, "%llu %llu %llu %u %llu %u %lf %lf %u %u %u", &ncu, &stride, &nrows, &num_hash, &alloc, &mixes, &density_max, &threshold, &flags, &bpc, &nknobs) == 11);
	for(unsigned k = 0; k < nknobs; ++k){
		char name[64];
		long long value;
		EXPECT(fscanf(f, "%63s %lld", name, &value) == 2);
		bool found = false;
		for(const Knob &kn : KNOBS){
			if(!strcmp(kn.name, name)){ tn.*kn.field = value; found = true; }
		}
		EXPECT(found);
	}
	EXPECT(fscanf(f, "%u", &ngroups) == 1);
	std::vector<uint64_t> pos_off(1, 0);
	uint64_t max_pos = 0;
	for(unsigned gi = 0; gi < ngroups; ++gi){
		unsigned count;
		unsigned long long npos;
		EXPECT(fscanf(f, "%u %llu", &count, &npos) == 2);
		for(unsigned i = 0; i < count; ++i){ pos_off.push_back(pos_off.back() + npos); }
		if(count){ max_pos = std::max<uint64_t>(max_pos, npos); }
	}
	in.ncu = ncu; in.stride = stride; in.nrows = nrows; in.num_hash = num_hash; in.alloc_bytes = alloc; in.mixes_regions = mixes != 0;
	in.density_max = density_max;
	in.n_queries = (uint32_t)(pos_off.size() - 1);
	in.total_pos = pos_off.back();
	in.max_pos = max_pos;
	in.h_pos_off = pos_off.data();
	in.threshold = (float)threshold;
	in.flags = flags;
	blocks_per_cu = bpc;
	in.count_screen_blocks_per_cu = screen_blocks;

	// the tables in allocations of exactly their size, and only where the plan says it fills them
	const bool fills = search_plan_fills_trunc_tables(tn, in);
	const uint32_t n = in.n_queries;
	std::string first;
	SearchPlan p;
	int rc = KWAGE_OK;
	std::vector<uint64_t> soff_kept;
	std::vector<uint32_t> kcut_kept;
	for(int pass = 0; pass < 2; ++pass){
		uint64_t *soff = fills ? new uint64_t[n + 1] : nullptr;
		uint32_t *kcut = fills ? new uint32_t[n] : nullptr;
		rc = plan_search(tn, in, soff, kcut, p);
		const std::string line = show(rc, p);
		if(pass == 0){
			first = line;
			if(fills){ soff_kept.assign(soff, soff + n + 1); kcut_kept.assign(kcut, kcut + n); }
		}
		else{
			EXPECT(line == first);       // deterministic
			if(fills){ EXPECT(!memcmp(soff, soff_kept.data(), (n + 1)*sizeof(uint64_t)) && !memcmp(kcut, kcut_kept.data(), n*sizeof(uint32_t))); }
		}
		delete[] soff;
		delete[] kcut;
	}
	if(rc != KWAGE_OK){ ++refused; }
	if(fills){
		++tables;
		// kcut[i] <= npos[i], slot_off the prefix sum of kcut
		EXPECT(soff_kept[0] == 0);
		for(uint32_t i = 0; i < n; ++i){
			EXPECT(kcut_kept[i] <= pos_off[i + 1] - pos_off[i]);
			EXPECT(soff_kept[i + 1] == soff_kept[i] + kcut_kept[i]);
		}
		if(rc == KWAGE_OK && p.form == SearchForm::COUNT_WALK_TRUNC){ EXPECT(p.total_slots == (uint64_t)p.chunks*soff_kept[n]); }
	}
	EXPECT((rc == KWAGE_OK && p.form == SearchForm::COUNT_WALK_TRUNC) ? fills : true);
	printf("case %ld %s\n", id, first.c_str());
	return 0;
}

int main(int argc, char **argv)
{
	if(argc != 2){ fprintf(stderr, "usage: search_plan_sanitize CASES.txt\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if(!f){ perror(argv[1]); return 2; }
	long id = -1;
	// the refusals no batch of a case file reaches (2^29 queries and more; a pairing the plan never makes): codes and texts
	EXPECT(check_launch_size(0x7FFFFFFFull*4 - 1, 1, 1) == KWAGE_OK);
	EXPECT(check_launch_size(0x7FFFFFFFull*4, 1, 1) == KWAGE_ERR_ARG && !strcmp(kwage_last_error(), "batch too large for one launch"));
	EXPECT(check_refine_units(14, 14) == KWAGE_OK && check_refine_units(10, 7) == KWAGE_OK);
	EXPECT(check_refine_units(10, 14) == KWAGE_ERR_STATE && !strcmp(kwage_last_error(), "count refine: 14-plane units with 10 counter planes"));
	while(fscanf(f, "%ld", &id) == 1){
		if(run_case(f, id)){ fclose(f); return 1; }
	}
	fclose(f);
	printf("sanitizers: %ld checks, %ld refusals, %ld truncation tables, no report\n", checks, refused, tables);
	return 0;
}
