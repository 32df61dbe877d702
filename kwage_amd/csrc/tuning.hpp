// kwage_amd/csrc/tuning.hpp -- what the kernels (kernels.hpp), the device library's state (engine_state.hpp) and the
// host-side plan of the gather stage (search_plan.hpp) share without a device: the kernel-selection knobs of a context and
// the launch constants of the search kernels, each defined here and nowhere else.  No HIP header: g++ alone compiles it.
#ifndef KWAGE_AMD_TUNING_HPP
#define KWAGE_AMD_TUNING_HPP

#include <cstdint>

namespace kwage {

static constexpr int WAVE = 64;
static constexpr int SEARCH_THREADS = 256;          // 4 waves, one tile each
static constexpr int WALK_WG_WAVES = 8;        // waves per workgroup (= per CU) of a chip-filling launch of the persistent kernels
static constexpr uint32_t BAND_MAX = 64;       // most bands of and_band_walk_kernel (BandArgs::bands)
static constexpr uint32_t CWALK_LEVELS = 32;      // tree depth a 32-bit wave count can need (count_walk_kernel)
static constexpr uint32_t REFINE_UNIT_BYTES = 32;     // sizeof(RefineUnit), kernels.hpp

// Kernel-selection knobs.  They are parsed ONCE, from the environment, when a context is created, and changed afterwards
// only through kwage_ctx_set_tuning (tests and tuning tools): nothing on the search path reads the environment.
struct Tuning {
	int64_t walk = 4;               // KWAGE_WALK: 0 = never the walk form (always the tiled kernel)
	int64_t walk_min_rows = -1;     // KWAGE_WALK_MIN_ROWS: batches with fewer rows use the tiled kernel (-1: 64 rows per wave of the chip)
	int64_t walk_max_kib = 16;      // KWAGE_WALK_MAX_KIB: widest row the walk form takes, in KiB-steps (wider rows: the tiled kernel's wide shape, which stays 0.5-3 % ahead on C3 / C4 and C3 split in two; the walk form handles them column tile after column tile when the knob is raised)
	int64_t walk_tile_kib = 16;     // KWAGE_WALK_TILE_KIB: widest column tile of the walk form in KiB-steps (rows wider than it are walked tile after tile)
	int64_t walk_min_kib = 2;       // KWAGE_WALK_MIN_KIB: narrowest row (in KiB-steps) the walk form takes (round 4: 2 -- rows of 1-2 KiB no
	                                //   longer need the tiled kernel's segments + combine pass: 0.263 vs 0.284 ms at C2's columns split 8 ways)
	int64_t walk_waves = 0;         // KWAGE_WALK_WAVES: exactly this many waves (tests: shares of every size); 0 = from the CU count
	int64_t walk_one_wg_per_cu = 1; // KWAGE_WALK_ONE_WG_PER_CU: chip-filling launches of the persistent kernels use one workgroup of 8 waves per CU (0: workgroups of 4 waves, placed by the dispatcher)
	int64_t walk_bands = -1;        // KWAGE_WALK_BANDS: the walk form takes the rows band after band of the matrix, all waves together (and_band_walk_kernel):
	                                //   -1 = three bands where the loader's probe found that the matrix's block mixes regions of the device's memory
	                                //   (the windowed probe > 3 % faster than the plain one), 0 = never, 2..64 = always, that many
	int64_t walk_bands_min_gib = 48;    // KWAGE_WALK_BANDS_MIN_GIB: a forced band count applies to matrices of at least this size
	int64_t and_vec = 0;            // KWAGE_AND_VEC: 16-byte vectors per lane of the tiled AND kernel (1, 2, 4; 0 = by row width)
	int64_t and_wide_min_kib = 16;  // KWAGE_AND_WIDE_MIN_KIB: ... for rows above this many KiB-steps (the walk form takes rows up to walk_max_kib first)
	int64_t and_wide = 1;           // KWAGE_AND_WIDE: rows beyond the walk form's range, no early exit, a chip-filling launch: vec 4, 8 rows, 8 waves per CU (and_config)
	int64_t narrow = 1;             // KWAGE_NARROW: several queries per wave for rows <= 512 B
	int64_t force_segs = 0;         // KWAGE_FORCE_SEGS: cut every query's k-mer list into this many segments (tests)
	int64_t scores_form = 0;        // KWAGE_SCORES_FORM: the dense score search's store epilogue (scores_kernels.hpp): 0 = a KiB of consecutive cells per store
	                                //   instruction, the planes crossing lanes through LDS; 1 = every lane stores its own 512-byte run (at C2 the first is the faster by just under 1 %: profiles/r06_scores_bench.txt)
	int64_t ee_refine = 1;          // KWAGE_EE_REFINE: with early exit, tiles that still hold a candidate column after the first rows are handed over to the
	                                //   refine launch, which reads 128-byte groups on a balanced grid (0: the tile's own wave walks on 1-2 KiB wide)
	int64_t refine_seg_rows = 32;   // KWAGE_REFINE_SEG_ROWS: rows (k-mers at t < 1) per unit of the refine launch (t < 1: at most 120).  32: four units for what is left of a 150-base read
	                                //   (100 k reads: 2.29 vs 2.48 with 64 and 3.18 with 128; 1 kb queries the same with all three -- profiles/r05_refine_knobs_ab.txt)
	int64_t refine_min_rows = 32;   // KWAGE_REFINE_MIN_ROWS: a tile with fewer rows (k-mers) left finishes by itself
	int64_t refine_max_groups = 4;  // KWAGE_REFINE_MAX_GROUPS: a tile is handed over once at most this many of its 128-byte groups hold a candidate column
	int64_t refine_unroll = 8;      // KWAGE_REFINE_UNROLL: rows in flight per 128-byte group in the refine launch (8 or 16)
	int64_t screen_wpc = 20;        // KWAGE_SCREEN_WPC: waves per CU of the persistent screen launch
	int64_t count_screen_wpc = 32;  // KWAGE_COUNT_SCREEN_WPC: at most this many waves per CU in the count path's screen launch (fewer where the kernel's registers hold fewer)
	int64_t count_screen_min_tiles = 8192;  // KWAGE_COUNT_SCREEN_MIN_TILES: at t < 1, batches with fewer (query, KiB tile) pairs keep the tiled kernel and its segments
	int64_t count_trunc = 1;        // KWAGE_COUNT_TRUNC: early exit over few long queries at t < 1: the persistent count kernel over the first k-mers of every
	                                //   query (as many as the bound needs before it can rule a column out), the survivors refined (0: segments, every row read)
	int64_t count_screen_check = 8;     // KWAGE_COUNT_SCREEN_CHECK: k-mers between two looks at the bound in the count path's screen launch (8, 16, 32, 64; 8 = after every step:
	                                //   short reads at t = 0.8 9 % sooner than with 16, 14 % sooner than with 32; C2 at t = 0.8 the same -- profiles/r05_refine_knobs_ab.txt)
	int64_t refine_static = 1;      // KWAGE_REFINE_STATIC: half of every list is dealt out to the screen launch's waves beforehand (0: every place is reserved through the counters -- diagnostics: kwage_ctx_refine_stats then counts the hand-overs exactly)
	int64_t refine_list_cap = 0;    // KWAGE_REFINE_LIST_CAP: capacity of each of the three lists of handed-over tiles (0 = from the batch; tests: full lists)
	int64_t count_walk = 1;         // KWAGE_COUNT_WALK: the persistent count kernel where it applies
	int64_t count_walk_wpc = 8;     // KWAGE_COUNT_WALK_WPC: its waves per CU (8: 6335 GB/s at C2's shape, 12: 6271, 16: 6250, 20: 5876)
	int64_t count_walk_waves = 0;   // KWAGE_COUNT_WALK_WAVES: exactly this many waves (tests)
	int64_t count_walk_min_rows = -1;   // KWAGE_COUNT_WALK_MIN_ROWS: smaller batches use the tiled kernel (-1: 64 rows for each of its waves)
	int64_t hit_sort_host = 0;      // KWAGE_HIT_SORT=host: order long hit lists on the host (A/B runs, the fallback)
	int64_t hit_copy_piece_kb = 0;  // KWAGE_HIT_COPY_PIECE_KB: piece size of the copy-back of a long hit list (0 = default)
	int64_t ext_launch_events = 1;  // KWAGE_EXT_LAUNCH_EVENTS: a gather stage's start / end events ride on its kernel launches (hipExtLaunchKernelGGL: no
	                                //   barrier packets between consecutive gather kernels); 0 = plain hipEventRecord around the stage
	int64_t shared_table_log2 = 0;  // KWAGE_SHARED_TABLE_LOG2: at least this many slots in a sample's shared distinct set (tests)
	// where a group's matrix lies (loader.hip, allocate_matrix) -- read when a group is created
	int64_t group_contiguous = 1;   // KWAGE_GROUP_CONTIGUOUS: ask for a physically contiguous block first (0: plain hipMalloc)
	int64_t group_placement_probe = 1;  // KWAGE_GROUP_PLACEMENT_PROBE: where two candidate blocks fit, time the gather pattern on both and keep the
	                                //   faster (+3-4 % at C2's shape); releasing the other costs ~3 s per 100 GB (the driver wipes it), so one-shot programs turn it off
	// the overlap matrix (overlap_plan.hpp overlap_choose_splits)
	int64_t overlap_splits = 0;     // KWAGE_OVERLAP_SPLITS: parts the row range is cut into (0 = the plan's choice; tests: 1, 2, 3 and 8 parts of 1024 rows)
	// the nearest-neighbour lists (neighbors_plan.hpp neighbors_strip_entries)
	int64_t neighbors_strip_bytes = 256ll << 20;   // KWAGE_NEIGHBORS_STRIP_BYTES: the cells of a strip of a's list fit this many bytes (tests: several strips)
};

}  // namespace kwage

#endif
