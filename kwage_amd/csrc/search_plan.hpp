// kwage_amd/csrc/search_plan.hpp -- the host-side planning of a threshold search's gather stage (engine.hip,
// launch_search_stage executes it): which form runs, its template integers, segments, launch shapes, list capacities and
// buffer sizes, the truncated walk's per-query tables, the refusals, and the name the search reports.  Plain functions of
// plain values: no device, no slot, no group -- tests/sanitize/search_plan_sanitize.cpp drives them under the sanitizers,
// and tests/test_search_plan.py checks the planned name of every case of tests/search_shapes.py without a GPU.
#ifndef KWAGE_AMD_SEARCH_PLAN_HPP
#define KWAGE_AMD_SEARCH_PLAN_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "internal.h"
#include "tuning.hpp"

namespace kwage {

// counter planes for counts up to `max_count`: the smallest instantiated size (7, 10, 14, 20 or 32) whose bits hold it
inline uint32_t planes_for(uint64_t max_count)
{
	uint32_t bits = 1;
	while(bits < 32 && (max_count >> bits) != 0){ ++bits; }
	return (bits <= 7) ? 7 : (bits <= 10) ? 10 : (bits <= 14) ? 14 : (bits <= 20) ? 20 : 32;
}

// How many segments to cut each query's k-mer list into, for a launch of n_queries lists over `chunks` tiles each: none
// while the launch already has enough waves to fill the chip; otherwise enough to reach ~TARGET_TILES waves (about 8 per CU, ~2x the bytes in flight that cover HBM latency), but never segments
// shorter than MIN_SEG_KMERS k-mers, and at most max_segs.  The force_segs knob forces a count (tests).
struct Segments { uint32_t segs, seg_kmers; };
inline Segments choose_segments(uint64_t n_queries, uint32_t chunks, uint64_t max_kmers, uint64_t max_segs, int64_t force_segs)
{
	static const uint64_t TARGET_TILES = 2048, MIN_SEG_KMERS = 64;
	Segments s = {1, (uint32_t)std::max<uint64_t>(max_kmers, 1)};
	uint64_t want = 1;
	if(force_segs > 0){ want = (uint64_t)force_segs; }
	else{
		const uint64_t tiles = n_queries*chunks;
		if(tiles >= TARGET_TILES || max_kmers < 2*MIN_SEG_KMERS){ return s; }
		want = std::min<uint64_t>((TARGET_TILES + tiles - 1)/tiles, max_kmers/MIN_SEG_KMERS);
	}
	want = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(want, max_segs), std::max<uint64_t>(max_kmers, 1)));
	if(want <= 1){ return s; }
	s.seg_kmers = (uint32_t)((max_kmers + want - 1)/want);
	s.segs = (uint32_t)((max_kmers + s.seg_kmers - 1)/s.seg_kmers);
	return s;
}

// The segment limit of a launch of the threshold search: its combine kernels index queries with gridDim.y, so no segments
// above 65535 queries.
inline uint64_t max_segments(uint64_t n_queries, uint64_t max_segs) { return (n_queries > 65535) ? 1 : max_segs; }

// The refusal of a launch whose tiles, four to a workgroup, do not fit a grid.
inline int fail_launch_size() { return fail(KWAGE_ERR_ARG, "batch too large for one launch"); }
inline int check_launch_size(uint64_t n_queries, uint32_t segs, uint32_t chunks)
{
	return (n_queries*segs*chunks/4 + 1 > 0x7FFFFFFFull) ? fail_launch_size() : KWAGE_OK;
}

// One value per branch of the dispatch that ends in a launch.  The tiled forms run with segments (and a combine launch)
// where SearchPlan::segs > 1.
enum class SearchForm {
	AND_NARROW, AND_SCREEN, AND_BAND_WALK, AND_WALK, AND_TILED,
	COUNT_SCREEN, COUNT_WALK_TRUNC, COUNT_WALK, COUNT_NARROW, COUNT_TILED
};

// What the dispatch knows of the group, the batch and the call.
struct SearchInputs {
	uint64_t ncu = 1;               // compute units of the device
	uint64_t stride = 0, nrows = 0; // bytes per row (a multiple of 128), rows of the matrix
	uint32_t num_hash = 1;
	uint64_t alloc_bytes = 0;       // size of the matrix's block, and whether the loader's probe found it mixing regions of the device's memory
	bool mixes_regions = false;
	double density_max = 1.0;       // share of set bits in the densest column (sampled at finalize)
	uint32_t n_queries = 0;
	uint64_t total_pos = 0, max_pos = 0;
	const uint64_t *h_pos_off = nullptr;    // n_queries + 1: position prefix (read by the truncated count walk only)
	float threshold = 1.0f;
	uint32_t flags = 0;
	// the one number asked of the device: workgroups of count_screen_kernel<planes, nh> a CU holds at once
	uint32_t (*count_screen_blocks_per_cu)(uint32_t planes, uint32_t nh) = nullptr;
};

// A list of the early-exit forms (kernels.hpp RefineList, field by field) ...
struct ListPlan { uint32_t cap, stat, base, chunk; };
// ... and everything refine_plan sizes: the scalars of RefineArgs, the three lists, bytes per item and per unit
// (unit_bytes 0: no slab), and the refine and emit launches.
struct RefinePlan {
	uint32_t seg_rows = 0, min_rows = 0, max_groups = 0, queue_batch = 0, check_every = 0;
	ListPlan lc = {}, li = {}, lu = {};         // clusters, items, units
	uint64_t clusters = 0, items = 0, units = 0, item_bytes = 0, unit_bytes = 0;
	uint32_t refine_wgs = 0, emit_wgs = 0;
};

struct SearchPlan {
	SearchForm form = SearchForm::AND_TILED;
	// the template integers of the form (those it does not have stay 0)
	int vec = 0, unroll = 0, up = 0;
	uint32_t ch = 0, G = 0, planes = 0, seg_planes = 0, tplanes = 0;
	uint32_t nh = 0, num_hash = 0;  // the instantiated hash count (1 to 4, 5 for five and more) and the group's own
	uint32_t segs = 1, seg_kmers = 0, chunks = 0;
	// the form's first launch: workgroups, waves per workgroup, dynamic LDS (a persistent launch's pad, the wide shape's cap)
	uint32_t wgs = 0, wg_waves = 0;
	size_t lds = 0;
	uint32_t combine_wgs = 0;       // the x extent of the combine launch's grid (segs > 1)
	uint32_t finish_wgs = 0;        // and_band_finish_kernel's grid
	uint32_t bands = 0, rows_per_band = 0;
	uint64_t total_slots = 0, per_wave = 0;     // persistent forms: the batch's (tile, position) slots and a wave's share
	RefinePlan refine;              // early-exit forms
	// bytes of the buffers the form needs (0: not needed)
	uint64_t partial_bytes = 0;     // segments: masks (AND) or partial counters (count)
	uint64_t exchange_bytes = 0;    // persistent forms: the cut pairs' meeting place (walk_or, band_or, cwalk_slab)
	uint64_t flags_bytes = 0;       // ... and its flags (walk_done, band_state, cwalk_arrived)
	uint64_t band_rows_bytes = 0, band_loc_bytes = 0;
	uint64_t trunc_bytes = 0;       // the truncated walk's tables: [slot_off: (n + 1) x u64 | kcut: n x u32]
	// truncated count walk: the per-k-mer match probability it was planned with, the unit length
	double trunc_pm = 0;
	uint64_t seg = 0;
};

static const uint32_t WALK_MIN_ROWS_PER_WAVE = 64;   // and_walk_kernel: below this share per wave the tiled kernel is used
static const uint32_t WALK_WAVES_PER_CU = 8;         // 2 workgroups: 2048 waves measured 1-2 % faster than 4096 (half the cut pairs)
static const int COUNT_NARROW_KPS = 8;               // k-mers per step of count_narrow_kernel (reported in its name)

// Waves a persistent launch wants: the knob's count (tests), else the chip's, fewer when the batch is small -- a wave
// should have WALK_MIN_ROWS_PER_WAVE rows to walk.
inline uint64_t persistent_waves(int64_t knob_waves, uint64_t chip_waves, uint64_t slots, uint32_t num_hash)
{
	return (knob_waves > 0) ? std::min<uint64_t>((uint64_t)knob_waves, slots)
		: std::max<uint64_t>(1, std::min<uint64_t>(chip_waves, slots*num_hash/WALK_MIN_ROWS_PER_WAVE));
}

// Launch shape of a persistent kernel that wants `want_waves` waves.  A chip-filling launch (8 waves per CU) uses ONE
// workgroup of 8 waves per CU -- a dynamic-LDS pad of more than half a CU's LDS keeps a second workgroup off --, so
// that every CU runs exactly 8 waves; smaller launches use workgroups of four waves wherever the dispatcher puts them.
struct WalkShape { uint32_t wgs, wg_waves; size_t lds; };
static const size_t WALK_PAD_LDS = 100*1024;

inline WalkShape walk_shape(const Tuning &tn, uint64_t want_waves, uint64_t ncu)
{
	WalkShape w;
	const bool pinned = tn.walk_one_wg_per_cu && want_waves == ncu*WALK_WG_WAVES;
	w.wg_waves = pinned ? (uint32_t)WALK_WG_WAVES : 4u;
	w.wgs = (uint32_t)((want_waves + w.wg_waves - 1)/w.wg_waves);
	w.lds = pinned ? WALK_PAD_LDS : 0;
	return w;
}

// ... set into the plan with the share of a wave; returns the launch's waves
inline uint64_t set_persistent(SearchPlan &p, const Tuning &tn, uint64_t want_waves, uint64_t ncu, uint64_t slots)
{
	const WalkShape shape = walk_shape(tn, want_waves, ncu);
	const uint64_t waves = (uint64_t)shape.wgs*shape.wg_waves;
	p.wgs = shape.wgs; p.wg_waves = shape.wg_waves; p.lds = shape.lds;
	p.total_slots = slots;
	p.per_wave = (slots + waves - 1)/waves;
	return waves;
}

// Shape of the tiled AND kernel: VEC 16-byte vectors per lane (by row width; knob and_vec), and -- the WIDE shape only -- a
// dynamic-LDS pad that caps the waves per CU.  Eight rows in flight and nontemporal loads always.
struct AndCfg { int vec, lds_bytes; };

// `wide`: rows beyond the walk form's range searched without early exit by a launch that fills the chip (C3, C4 and their
// column shares): four vectors per lane, eight rows in flight, and a dynamic-LDS pad that keeps 8 waves per CU resident
// -- 32 KiB in flight per wave, 256 KiB per CU.  As for the persistent kernels, the memory system prefers few deep
// streams to many: against the default shape (32 waves per CU, 16 KiB each) +1.4 % on C3 and on the C4 share in one
// process (12 waves per CU +0.4 %, 16 and 20 the same as the default, 4 waves per CU -20 %; profiles/r04_tune_and_wide_rows.txt).
inline AndCfg and_config(const Tuning &t, uint32_t units_per_row, bool wide = false)
{
	AndCfg c;
	if(wide && t.and_vec == 0){ c.vec = 4; c.lds_bytes = 80*1024; return c; }
	c.vec = (t.and_vec == 1 || t.and_vec == 2 || t.and_vec == 4) ? (int)t.and_vec : ((units_per_row >= 4*WAVE) ? 2 : 1);
	c.lds_bytes = 0;
	return c;
}

// Units of 14 planes (up == 14) pair count_refine_kernel<NH, 14> with count_refine_emit_kernel<P, 14>, which exists for
// P >= 14 only: any other pairing would read the slab with a stride it was not written with.  Checked before the first
// launch of the stage.
inline int check_refine_units(uint32_t planes, int up)
{
	if(up == 14 && planes < 14){ return fail(KWAGE_ERR_STATE, "count refine: 14-plane units with %u counter planes", planes); }
	return KWAGE_OK;
}

// k-mers per unit of the count path's refine launch before the batch's lengths are looked at: the refine_seg_rows knob,
// 8 to 120 in steps of 8 (7 counter planes per unit hold 120)
inline uint32_t refine_unit_len(const Tuning &tn)
{
	return (uint32_t)std::min<int64_t>(std::max<int64_t>(tn.refine_seg_rows, 8), 120)/8*8;
}

// The lists of the early-exit form "screen, then refine" (kernels.hpp and_screen_kernel), sized from the batch: room for
// eight handed-over 128-byte groups per query (three planted columns per query is what the synthetic workloads hold; a
// tile that finds the lists full walks on by itself) and for the units of as many items of average length.  Half of
// every list is static -- its places dealt out to the `screen_waves` waves of the screen launch beforehand, taken without an
// atomic --, the rest is reserved in chunks through three counters, zeroed on the gather stream before every stage.
// `item_bytes`: mask (t = 1: 128) or counters (t < 1: planes x 128) per item; `unit_bytes`: partial counters per unit
// (t < 1 only).  exact_*: the truncated count walk names its capacities (exact_units 0: sized here).
inline void refine_plan(const Tuning &tn, uint32_t n_queries, uint64_t total_rows, uint64_t max_rows, uint32_t max_seg, uint64_t item_bytes, uint64_t unit_bytes,
                        uint64_t tiles, uint64_t screen_waves, uint64_t ncu, RefinePlan &r,
                        uint64_t exact_clusters = 0, uint64_t exact_items = 0, uint64_t exact_units = 0)
{
	r.seg_rows = (uint32_t)std::min<int64_t>(std::max<int64_t>(tn.refine_seg_rows, 8), max_seg);
	r.seg_rows = (uint32_t)std::max<uint64_t>(r.seg_rows, (max_rows + 65535)/65536);              // (at most 2^16 units per item; the count path passes its own segment length)
	r.min_rows = (uint32_t)std::max<int64_t>(tn.refine_min_rows, 1);
	r.max_groups = (uint32_t)std::min<int64_t>(std::max<int64_t>(tn.refine_max_groups, 0), 16);      // (0: nothing is ever handed over)
	uint64_t items = std::min<uint64_t>(std::max<uint64_t>(8ull*n_queries, 1u << 16), 1u << 20);
	items = std::max<uint64_t>(std::min<uint64_t>(items, (256ull << 20)/item_bytes), 1024);
	uint64_t units = std::min<uint64_t>(std::max<uint64_t>(32*total_rows/r.seg_rows, 1u << 18), 1u << 25);       // (32 bytes each: at most 1 GiB)
	if(unit_bytes){ units = std::max<uint64_t>(std::min<uint64_t>(units, (512ull << 20)/unit_bytes), 4096); }
	if(tn.refine_list_cap > 0){ items = units = (uint64_t)std::min<int64_t>(tn.refine_list_cap, 1 << 20); }
	uint64_t clusters = items;
	// (the truncated count walk names its capacities: a place for every pair and group, units by memory)
	if(exact_units){ clusters = exact_clusters; items = exact_items; units = exact_units; }
	if(exact_units && tn.refine_list_cap > 0){ clusters = items = units = (uint64_t)std::min<int64_t>(tn.refine_list_cap, 1 << 20); }       // (tests: full lists)
	// dynamic chunks: what a wave is likely to need for a few of its tiles (a wave with one or two tiles takes exactly what it needs)
	const uint64_t tiles_per_wave = (tiles + screen_waves - 1)/std::max<uint64_t>(screen_waves, 1);
	auto list = [&](uint64_t cap, uint64_t stat_max, uint64_t chunk_max) {
		ListPlan ls;
		ls.cap = (uint32_t)cap;
		// (exact capacities: every place is taken exactly when it is needed -- no static parts, no chunks, nothing left unused)
		ls.stat = (tn.refine_static && !exact_units) ? (uint32_t)std::min<uint64_t>(stat_max, cap/2/std::max<uint64_t>(screen_waves, 1)) : 0u;
		ls.base = (uint32_t)(ls.stat*screen_waves);
		ls.chunk = exact_units ? 1u : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk_max, tiles_per_wave/4));
		return ls;
	};
	r.lc = list(clusters, 32, 32);
	r.li = list(items, 64, 64);
	r.lu = list(units, 256, 256);
	r.clusters = clusters; r.items = items; r.units = units;
	r.item_bytes = item_bytes; r.unit_bytes = unit_bytes;
	r.queue_batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(16, tiles/(8*std::max<uint64_t>(screen_waves, 1))));
	r.check_every = (tn.count_screen_check == 16 || tn.count_screen_check == 32 || tn.count_screen_check == 64) ? (uint32_t)tn.count_screen_check : 8u;
	r.refine_wgs = (uint32_t)(ncu*8);          // 32 waves per CU, eight units each
	r.emit_wgs = (uint32_t)(ncu*4);            // 16 waves per CU, four clusters at a time each
}

// The search at t = 1 (kwage.cpp:404-470): AND of the addressed rows.
inline int plan_and(const Tuning &tn, const SearchInputs &in, SearchPlan &p)
{
	const uint64_t ncu = std::max<uint64_t>(in.ncu, 1), n = in.n_queries;
	const uint32_t units_per_row = (uint32_t)(in.stride/16);
	const bool early_exit = (in.flags & KWAGE_SEARCH_EARLY_EXIT) != 0;
	const uint32_t whole_list = (uint32_t)std::max<uint64_t>(in.max_pos, 1);      // seg_kmers of a form that takes no segments
	int rc;
	// The wide shape of the tiled kernel (and_config) where a launch without early exit fills the chip with 4 KiB tiles: for
	// rows beyond the walk form's range.  (Within that range the walk form is ahead for every row-list length since its
	// waves buffer their hit records: a rule that sent batches of short row lists to the wide shape was dropped in round 4,
	// its knob in round 5; profiles/r04_walk_vs_tiled_wide_grid.txt, r04_walk_hit_cost.txt.)
	const uint64_t wide_tiles = n*((units_per_row + 4*WAVE - 1)/(4*WAVE));
	const bool wide_ok = tn.and_wide && !early_exit && wide_tiles >= 8*ncu;
	const bool wide_rows = wide_ok && units_per_row > (uint32_t)std::max<int64_t>(tn.and_wide_min_kib, 1)*WAVE;
	const AndCfg cfg = and_config(tn, units_per_row, wide_rows);
	p.chunks = (units_per_row + WAVE*cfg.vec - 1)/(WAVE*cfg.vec);
	const Segments sg = choose_segments(n, p.chunks, in.max_pos, max_segments(n, 4096), tn.force_segs);
	p.segs = sg.segs; p.seg_kmers = sg.seg_kmers;
	if((rc = check_launch_size(n, p.segs, p.chunks))){ return rc; }
	// narrow rows: several queries per wave (tools/bench_narrow.py)
	if(tn.narrow && p.segs == 1 && units_per_row <= 32 && n >= 64){
		p.form = SearchForm::AND_NARROW;
		p.G = (units_per_row <= 4) ? 16 : (units_per_row <= 8) ? 8 : (units_per_row <= 16) ? 4 : 2;
		const uint64_t waves = (n + p.G - 1)/p.G;
		p.wgs = (uint32_t)((waves + 3)/4); p.wg_waves = SEARCH_THREADS/WAVE;
		// few waves (10 k queries of 1 kb: ten per CU): sixteen rows in flight per wave instead of eight
		p.unroll = (waves < ncu*16) ? 16 : 8;
		return KWAGE_OK;
	}
	// early exit on rows of a KiB and more: screen, then refine (kernels.hpp and_screen_kernel)
	if(early_exit && tn.ee_refine && units_per_row >= WAVE && tn.force_segs <= 0){
		p.form = SearchForm::AND_SCREEN;
		p.vec = (units_per_row >= 4*WAVE) ? 2 : 1;
		p.segs = 1; p.seg_kmers = whole_list;
		p.chunks = (units_per_row + WAVE*p.vec - 1)/(WAVE*p.vec);
		const uint64_t tiles = n*p.chunks;
		// (a persistent grid: tile t goes to wave t mod waves; 20 waves per CU is what the kernel's registers allow)
		const uint64_t screen_waves = (std::min<uint64_t>(tiles, ncu*(uint64_t)std::max<int64_t>(tn.screen_wpc, 1)) + 3)/4*4;
		refine_plan(tn, in.n_queries, in.total_pos*in.num_hash, in.max_pos*in.num_hash, 1u << 20, 128, 0, tiles, screen_waves, ncu, p.refine);
		p.unroll = (tn.refine_unroll == 16) ? 16 : 8;
		p.wgs = (uint32_t)(screen_waves/4); p.wg_waves = SEARCH_THREADS/WAVE;
		return KWAGE_OK;
	}
	// rows of 3..16 KiB: the walk form (a persistent grid, every wave walks an equal share of the batch's row
	// list over the whole width of a column tile; kernels.hpp and_walk_kernel).  Worth it once every wave of
	// the chip gets a few dozen rows; smaller batches stay with the tiled kernel and its row-list segments.
	const uint64_t walk_min_rows = (tn.walk_min_rows >= 0) ? (uint64_t)tn.walk_min_rows : (uint64_t)WALK_MIN_ROWS_PER_WAVE*256*WALK_WAVES_PER_CU;
	const uint32_t kib = (units_per_row + WAVE - 1)/WAVE;
	// (the kernel handles wider rows as several balanced column tiles -- the walk_max_kib knob raises the limit --
	// but 125 KB rows measured no gain over the tiled kernel)
	const uint32_t walk_max_kib = (uint32_t)std::max<int64_t>(tn.walk_max_kib, 0);
	// (knob walk_tile_kib: narrower column tiles -- with 4, eight rows in flight and no pacing a wave requests 4 KiB of each
	// of eight rows at once: the tiled kernel's wide shape on the balanced persistent grid)
	const uint32_t walk_tile = (uint32_t)std::min<int64_t>(std::max<int64_t>(tn.walk_tile_kib, 1), 16);
	const uint32_t coltiles = (kib + walk_tile - 1)/walk_tile, walk_ch = (kib + coltiles - 1)/coltiles;     // balanced tiles of <= walk_tile KiB
	// (early exit never comes here: a walking wave covers a column tile's whole width and has nothing to give up --
	// C2 with early exit measured 1.29 ms through the walk form against 0.64 ms tiled; the screen + refine form above
	// takes rows of a KiB and more, the tiled kernel below the rest)
	const bool walk_ee_ok = !early_exit;
	const uint64_t walk_slots = (uint64_t)coltiles*in.total_pos;
	const uint32_t walk_min_kib = (uint32_t)std::max<int64_t>(tn.walk_min_kib, 1);
	if(tn.walk && walk_ee_ok && kib >= walk_min_kib && kib <= walk_max_kib && walk_slots*in.num_hash >= walk_min_rows && walk_slots > 0){
		// WALK_WAVES_PER_CU waves per CU, all resident at once (__launch_bounds__(256, 4) allows twice as many),
		// fewer when the batch is small: a wave should have WALK_MIN_ROWS_PER_WAVE rows to walk
		const uint64_t waves = set_persistent(p, tn, persistent_waves(tn.walk_waves, ncu*WALK_WAVES_PER_CU, walk_slots, in.num_hash), ncu, walk_slots);
		p.ch = walk_ch;
		p.segs = 1; p.seg_kmers = whole_list;
		p.chunks = coltiles;
		// Band after band (and_band_walk_kernel): matrices large enough to span several regions of the device's memory,
		// one column tile, a slot of 16 KiB per query affordable.  (With early exit the tiled kernel is the default anyway.)
		const uint64_t band_items = in.total_pos*in.num_hash;
		// (a matrix of at least walk_bands_min_gib either way: the probe's "mixes regions" on a 14 GB matrix of 1.6 KB rows --
		// C2's columns split 8 ways -- sent that shape through the band form at 2.8x the walk form's time)
		const bool big_enough = in.alloc_bytes >= ((uint64_t)std::max<int64_t>(tn.walk_bands_min_gib, 0) << 30);
		const uint32_t bands = !big_enough ? 0u : (tn.walk_bands < 0) ? (in.mixes_regions ? 3u : 0u) : (uint32_t)std::min<int64_t>(tn.walk_bands, BAND_MAX);
		// (rows of one or two KiB-steps stay with the plain walk form: the band kernels are instantiated for 3..16 KiB-steps)
		if(bands >= 2 && coltiles == 1 && walk_ch >= 3 && n*16*1024 <= (256ull << 20) && band_items < 0x7FFFFFFFull){
			p.form = SearchForm::AND_BAND_WALK;
			p.unroll = 4;
			p.bands = bands;
			p.rows_per_band = (uint32_t)((in.nrows + bands - 1)/bands);
			p.band_rows_bytes = band_items*sizeof(uint32_t);
			p.band_loc_bytes = n*(bands + 1)*sizeof(uint32_t);
			p.exchange_bytes = n*16*1024;
			p.flags_bytes = n*sizeof(uint32_t);
			p.finish_wgs = (in.n_queries + 3)/4;
			return KWAGE_OK;
		}
		p.form = SearchForm::AND_WALK;
		// rows in flight per wave: 4; 8 for rows of one or two KiB-steps (a group of four such rows is only 4-8 loads: C2's
		// columns split 8 ways, 1664-byte rows, 0.2626 vs 0.2667 ms)
		p.unroll = (walk_ch <= 2) ? 8 : 4;
		// cut-pair slots: one per wave, 16 KiB each whatever CH is; the kernel leaves them zero
		p.exchange_bytes = waves*16*1024;
		p.flags_bytes = waves*2*sizeof(uint32_t);
		return KWAGE_OK;
	}
	p.form = SearchForm::AND_TILED;
	p.vec = cfg.vec;
	p.lds = (size_t)cfg.lds_bytes;
	p.wgs = (uint32_t)((n*p.segs*p.chunks + SEARCH_THREADS/WAVE - 1)/(SEARCH_THREADS/WAVE)); p.wg_waves = SEARCH_THREADS/WAVE;
	if(p.segs > 1){
		p.partial_bytes = n*in.stride;
		p.combine_wgs = (units_per_row + 255)/256;
	}
	return KWAGE_OK;
}

// What the count path (t < 1) decides before any of its forms is sized.
struct CountGate {
	uint32_t units_per_row, chunks, planes;
	bool narrow, screen, trunc;     // narrow rows; the screen form runs; the truncated walk is considered (its tables are needed)
};
inline CountGate count_gate(const Tuning &tn, const SearchInputs &in)
{
	CountGate c;
	const bool early_exit = (in.flags & KWAGE_SEARCH_EARLY_EXIT) != 0;
	c.units_per_row = (uint32_t)(in.stride/16);
	c.chunks = (c.units_per_row + WAVE - 1)/WAVE;
	// counter planes: enough bits for the largest possible num_query_kmer of the batch
	c.planes = planes_for(in.max_pos);
	c.narrow = tn.narrow && c.units_per_row <= 32 && c.units_per_row > 8 && in.n_queries >= 64 && c.planes <= 14;
	const bool refine_ok = early_exit && tn.ee_refine && !c.narrow && tn.force_segs <= 0 && c.units_per_row >= WAVE;
	c.screen = refine_ok && (uint64_t)in.n_queries*c.chunks >= (uint64_t)std::max<int64_t>(tn.count_screen_min_tiles, 1) && c.planes <= 14;      // (queries of up to 16383 positions: 20 and 32 counter planes + eight rows in flight do not fit a wave's registers)
	c.trunc = !c.screen && refine_ok && tn.count_trunc && tn.count_walk && in.total_pos > 0;
	return c;
}

// Whether plan_search will fill the truncated walk's tables: the caller provides soff[n_queries + 1] and kcut[n_queries] then.
inline bool search_plan_fills_trunc_tables(const Tuning &tn, const SearchInputs &in)
{
	return in.threshold != 1.0f && count_gate(tn, in).trunc;
}

// The search at t < 1: bit-sliced counters per column.
inline int plan_count(const Tuning &tn, const SearchInputs &in, uint64_t *soff, uint32_t *kcut, SearchPlan &p)
{
	const uint64_t ncu = std::max<uint64_t>(in.ncu, 1), n = in.n_queries;
	const bool early_exit = (in.flags & KWAGE_SEARCH_EARLY_EXIT) != 0;
	const CountGate gate = count_gate(tn, in);
	const uint32_t planes = gate.planes;
	int rc;
	p.chunks = gate.chunks;
	p.planes = planes;
	p.seg_kmers = (uint32_t)std::max<uint64_t>(in.max_pos, 1);      // (one segment, the whole list, until the segments below)
	// The persistent form (count_walk_kernel): equal shares of the batch's (query, KiB tile, position) list per wave,
	// pairs cut by share boundaries added up as a tree through memory.  Taken when the batch gives every wave of the
	// launch its 64 rows and no early exit is asked for (a persistent wave has no tile of its own to give up): long
	// queries need no segment slab and no combine pass then (1 x 100 kb: 5410 vs 4813 GB/s, 4 x 1 Mb: 6431 vs 5705),
	// no batch size ends in a part-filled round of waves, and in a host's software pipeline its resident waves do not
	// share the CUs with the next batch's k-mer stage the way the tiled kernel's 13 000 workgroups do (C2 at t = 0.8
	// inside bench.py: 1.988 vs 2.077 ms, profiles/r03_c2t_bench_ab.txt).  (Alone on the chip, batches whose tiles
	// all fit in one round are 2-3 % faster through the tiled kernel -- 300 queries 0.582 vs 0.598 ms --: not worth
	// a rule of their own.)  Early exit, tiny batches and forced segment counts go on below.
	// early exit on rows of a KiB and more, enough (query, KiB tile) pairs to keep a persistent grid busy: screen, then refine
	// (kernels.hpp count_screen_kernel).  Few long queries stay with the segments below: every tile has to read the first
	// (1 - t) n k-mers before the bound can prune anything, and a handful of tiles that long would be the whole launch.
	if(gate.screen){
		p.form = SearchForm::COUNT_SCREEN;
		const uint64_t tiles = n*p.chunks;
		// k-mers per unit: 64 (7 counter planes per unit); queries above 8192 positions: 1/128 of the longest (14 planes)
		uint32_t seg = refine_unit_len(tn);
		p.up = 7;
		if(in.max_pos > 8192){ seg = (uint32_t)((in.max_pos + 127)/128 + 7)/8*8; p.up = 14; }
		// (as many waves as the kernel's registers let a CU hold -- knob count_screen_wpc caps it; they draw their tiles from a queue)
		const uint64_t wpc = std::min<uint64_t>((uint64_t)std::max<int64_t>(tn.count_screen_wpc, 1), 4ull*in.count_screen_blocks_per_cu(planes, p.nh));
		const uint64_t screen_waves = (std::min<uint64_t>(tiles, ncu*wpc) + 3)/4*4;
		if((rc = check_refine_units(planes, p.up))){ return rc; }
		refine_plan(tn, in.n_queries, in.total_pos, 0, seg, (uint64_t)planes*128, (uint64_t)p.up*128, tiles, screen_waves, ncu, p.refine);
		p.refine.seg_rows = seg;
		p.segs = 1;
		p.wgs = (uint32_t)(screen_waves/4); p.wg_waves = SEARCH_THREADS/WAVE;
		return KWAGE_OK;
	}
	// Early exit over FEW LONG queries (fewer tiles than the screen form wants, or more counter planes than it holds): every
	// tile has to read the first (1 - t) n k-mers plus a margin before kwage.cpp:478-481 can rule anything out, and a handful of
	// tiles that long would be the whole launch -- so that part is walked by the BALANCED persistent count kernel over the
	// first kcut(q) k-mers of every query (count_walk_kernel<.., TRUNC>), the columns that can still reach the threshold are
	// handed over with their counters, and the refine launch counts their remaining k-mers in 128-byte groups.  kcut comes
	// from the density of the matrix's DENSEST column (sampled at finalize): the smallest K with  K - (n - thr)  >=  pm K + 4.5 sqrt(pm (1 - pm) K) + 8,
	// pm = that density ^ num_hash -- an estimate that decides how much is read, never what is reported.
	if(gate.trunc){
		const uint32_t nq = in.n_queries;
		const uint32_t tplanes = std::max<uint32_t>(planes, 10);      // (no 7-plane instantiation of this form)
		// The DENSEST column decides: a 128-byte group stays alive while any of its 1024 columns can still reach the threshold,
		// and columns are not equally dense (every sample's filter has its own fill; the synthetic workloads' planted columns
		// are 15 % denser than the rest).  + 3 sigma of what 4096 sampled rows can say about one column.
		const double col = std::min(1.0, std::max(0.0, in.density_max) + 3.0*std::sqrt(0.25/4096.0));
		const double pm = std::min(0.9, std::max(0.0005, std::pow(col, (double)in.num_hash)));
		p.trunc_pm = pm;
		uint64_t walked = 0, max_rest = 0, rest_total = 0;
		soff[0] = 0;
		for(uint32_t i = 0; i < nq; ++i){
			const uint64_t npos = in.h_pos_off[i + 1] - in.h_pos_off[i];
			uint64_t kc = npos;
			if(npos >= 64){
				const uint32_t thr = (uint32_t)(in.threshold*(float)npos);      // kwage.cpp:388 on the positions (an upper bound of the distinct k-mers)
				const double need = (double)(npos - std::min<uint64_t>(thr, npos));
				double K = (need + 8.0)/(1.0 - pm);
				for(int it = 0; it < 8; ++it){ K = (need + 8.0 + 4.5*std::sqrt(pm*(1.0 - pm)*K))/(1.0 - pm); }
				const uint64_t k8 = ((uint64_t)K + 7)/8*8;
				if(k8*20 <= npos*17){ kc = k8; }                              // (worth it when at least 15 % of the list is left out)
			}
			kcut[i] = (uint32_t)kc;
			soff[i + 1] = soff[i] + kc;
			walked += kc;
			max_rest = std::max(max_rest, npos - kc);
			rest_total += npos - kc;
		}
		const uint64_t slots = (uint64_t)p.chunks*walked;
		const uint64_t chip_waves = ncu*(uint64_t)std::max<int64_t>(tn.count_walk_wpc, 1);
		const uint64_t min_rows = (tn.count_walk_min_rows >= 0) ? (uint64_t)tn.count_walk_min_rows : (uint64_t)WALK_MIN_ROWS_PER_WAVE*chip_waves;
		// units of 1/128 of the longest remainder (at least refine_seg_rows k-mers): 7 counter planes per unit up to 120 k-mers, 14 beyond
		const uint64_t seg = std::max<uint64_t>(refine_unit_len(tn), ((max_rest + 127)/128 + 7)/8*8);
		const int up = (seg <= 120) ? 7 : 14;
		uint64_t units_worst = 0;
		for(uint32_t i = 0; i < nq && seg; ++i){
			const uint64_t rest = (in.h_pos_off[i + 1] - in.h_pos_off[i]) - kcut[i];
			units_worst += (uint64_t)p.chunks*8*((rest + seg - 1)/seg);
		}
		// Lists: a place for every pair and every 128-byte group of it (few tiles: that is affordable), and for the units
		// as many as a GiB of partial counters holds -- every group of every pair surviving is not what they are sized for;
		// a pair that finds them full is counted to the end by the wave that holds it (count_walk_kernel).
		const uint64_t tiles = (uint64_t)nq*p.chunks;
		const uint64_t units_cap = std::max<uint64_t>(4096, std::min<uint64_t>(units_worst, (1ull << 30)/((uint64_t)up*128 + REFINE_UNIT_BYTES)));
		if(walked*10 <= in.total_pos*7 && slots*in.num_hash >= min_rows && seg <= 16376 && rest_total > 0 && tiles*8*(uint64_t)tplanes*128 <= (1ull << 30)){
			p.form = SearchForm::COUNT_WALK_TRUNC;
			p.tplanes = tplanes;
			p.up = up;
			p.seg = seg;
			const uint64_t waves = set_persistent(p, tn, persistent_waves(tn.count_walk_waves, chip_waves, slots, in.num_hash), ncu, slots);
			if((rc = check_refine_units(tplanes, up))){ return rc; }
			refine_plan(tn, nq, rest_total, 0, (uint32_t)seg, (uint64_t)tplanes*128, (uint64_t)up*128, tiles, waves, ncu, p.refine, tiles, tiles*8, units_cap);
			p.refine.seg_rows = (uint32_t)seg;
			p.trunc_bytes = ((uint64_t)nq + 1)*sizeof(uint64_t) + (uint64_t)nq*sizeof(uint32_t);
			p.exchange_bytes = waves*2*tplanes*1024;
			p.flags_bytes = waves*CWALK_LEVELS*sizeof(uint32_t);
			p.segs = 1;
			return KWAGE_OK;
		}
	}
	if(tn.count_walk && !early_exit && !gate.narrow && tn.force_segs <= 0 && in.total_pos > 0){
		const uint64_t slots = (uint64_t)p.chunks*in.total_pos;
		const uint64_t chip_waves = ncu*(uint64_t)std::max<int64_t>(tn.count_walk_wpc, 1);
		const uint64_t min_rows = (tn.count_walk_min_rows >= 0) ? (uint64_t)tn.count_walk_min_rows : (uint64_t)WALK_MIN_ROWS_PER_WAVE*chip_waves;
		if(slots*in.num_hash >= min_rows){
			// (shape: planes, hashes, the next step's rows prefetched, eight k-mers per step with 14 planes and more)
			p.form = SearchForm::COUNT_WALK;
			const uint64_t waves = set_persistent(p, tn, persistent_waves(tn.count_walk_waves, chip_waves, slots, in.num_hash), ncu, slots);
			p.exchange_bytes = waves*2*planes*1024;
			p.flags_bytes = waves*CWALK_LEVELS*sizeof(uint32_t);
			p.segs = 1;
			return KWAGE_OK;
		}
	}
	// Long queries: segments of the k-mer list are counted by different waves into a slab of partial counters
	// and added by count_combine_kernel (a tree per (query, 64 units)); a segment's counters need only the
	// planes its own k-mer count can reach.
	Segments sg = choose_segments(n, p.chunks, in.max_pos, max_segments(n, 1024), tn.force_segs);
	uint32_t seg_planes = (sg.segs > 1) ? planes_for(sg.seg_kmers) : planes;
	// keep the slab of partial counters bounded (1 GiB)
	while(sg.segs > 1 && n*sg.segs*seg_planes*in.stride > (1ull << 30)){
		const uint64_t want = sg.segs/2;
		sg.seg_kmers = (uint32_t)((in.max_pos + want - 1)/std::max<uint64_t>(want, 1));
		sg.segs = (uint32_t)((in.max_pos + sg.seg_kmers - 1)/sg.seg_kmers);
		seg_planes = (sg.segs > 1) ? planes_for(sg.seg_kmers) : planes;
	}
	p.segs = sg.segs; p.seg_kmers = sg.seg_kmers; p.seg_planes = seg_planes;
	if((rc = check_launch_size(n, p.segs, p.chunks))){ return rc; }
	p.wg_waves = SEARCH_THREADS/WAVE;
	if(p.segs > 1){
		p.partial_bytes = n*p.segs*seg_planes*in.stride;
		p.combine_wgs = (gate.units_per_row + WAVE - 1)/WAVE;
	}
	if(gate.narrow && p.segs == 1){
		// one reference file (<= 2048 columns = 16 units) or two: 4 resp. 2 queries per wave
		p.form = SearchForm::COUNT_NARROW;
		p.G = (gate.units_per_row <= 16) ? 4 : 2;
		p.wgs = (uint32_t)(((n + p.G - 1)/p.G + 3)/4);
		return KWAGE_OK;
	}
	p.form = SearchForm::COUNT_TILED;
	p.wgs = (uint32_t)((n*p.segs*p.chunks + 3)/4);
	return KWAGE_OK;
}

// The plan of one search.  soff / kcut: storage for the truncated walk's tables (n_queries + 1 and n_queries entries),
// written where search_plan_fills_trunc_tables() says so and unused otherwise.  Refusals are fail()'s codes and texts.
inline int plan_search(const Tuning &tn, const SearchInputs &in, uint64_t *soff, uint32_t *kcut, SearchPlan &p)
{
	p = SearchPlan();
	p.num_hash = in.num_hash;
	p.nh = std::min(in.num_hash, 5u);
	return (in.threshold == 1.0f) ? plan_and(tn, in, p) : plan_count(tn, in, soff, kcut, p);
}

// The name a search reports (kwage_result::search_kernel): the form's first kernel with its template shape.
inline void format_search_name(const SearchPlan &p, char *out, size_t n)
{
	switch(p.form){
		case SearchForm::AND_NARROW: snprintf(out, n, "and_narrow_kernel<%u,%d>", p.G, p.unroll); break;
		case SearchForm::AND_SCREEN: snprintf(out, n, "and_screen_kernel<%d,8>+refine<%d>", p.vec, p.unroll); break;
		case SearchForm::AND_BAND_WALK: snprintf(out, n, "and_band_walk_kernel<%u,4>", p.ch); break;
		case SearchForm::AND_WALK: snprintf(out, n, "and_walk_kernel<%u,%d>", p.ch, p.unroll); break;
		case SearchForm::AND_TILED: snprintf(out, n, "and_kernel<%d,8,nt>%s", p.vec, p.segs > 1 ? "+segments" : ""); break;      // (shape: vectors per lane, rows in flight, nontemporal)
		case SearchForm::COUNT_SCREEN: snprintf(out, n, "count_screen_kernel<%u,%u>+refine<%d>", p.planes, p.nh, p.up); break;
		case SearchForm::COUNT_WALK_TRUNC: snprintf(out, n, "count_walk_kernel<%u,%u,trunc>+refine<%d>", p.tplanes, p.nh, p.up); break;
		case SearchForm::COUNT_WALK: snprintf(out, n, "count_walk_kernel<%u,%u,pf%s>", p.planes, p.nh, p.planes >= 14 ? ",8" : ""); break;
		case SearchForm::COUNT_NARROW: snprintf(out, n, "count_narrow_kernel<%u,%u,%d,%d>", p.planes, p.num_hash, (int)p.G, COUNT_NARROW_KPS); break;
		case SearchForm::COUNT_TILED:
			if(p.segs > 1){ snprintf(out, n, "count_kernel<%u,%u>+segments->%u", p.seg_planes, p.nh, p.planes); }
			else{ snprintf(out, n, "count_kernel<%u,%u>", p.planes, p.nh); }
			break;
	}
}

}  // namespace kwage

#endif
