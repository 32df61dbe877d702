/* include/kwage_amd.h -- C ABI of the MI355X-native `kwage` search engine.
 *
 * This is the drop-in boundary for the one hot path of LANL-Bioinformatics/KWAGE: the body
 * of `search()` (reference kwage.cpp:26-31 declaration, :340-541 body) and the two loops in
 * `main` that call it (kwage.cpp:116-148).  The reference has no FFI of its own; a
 * maintainer replaces those loops with the calls below (INTEGRATION.md shows the patch).
 *
 * Conventions
 *   - plain C types only; every function returns KWAGE_OK (0) or a negative status and
 *     records a message retrievable with kwage_last_error() (thread local) -- this replaces
 *     the reference's `throw "file:func: msg"` literals (kwage.cpp:419,452; hash.cpp:92).
 *   - objects are opaque handles, created/destroyed explicitly; buffers returned by the
 *     library stay owned by it until the matching free / destroy call.
 *   - one kwage_ctx == one GPU == one HIP stream.  A ctx and the objects made from it may be
 *     used from one thread at a time; different ctxs are independent (this mirrors the
 *     reference's per-OpenMP-thread ifstream + result map, kwage.cpp:76-89).
 *   - there is NO CPU fallback: without a usable gfx950 device kwage_init fails.
 */
#ifndef KWAGE_AMD_H
#define KWAGE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KWAGE_AMD_ABI_VERSION 1

enum {
	KWAGE_OK = 0,
	KWAGE_ERR_ARG = -1,        /* bad argument / unsupported parameter                    */
	KWAGE_ERR_DEVICE = -2,     /* HIP error (no device, out of memory, launch failure)    */
	KWAGE_ERR_IO = -3,         /* file could not be opened / read / is truncated          */
	KWAGE_ERR_FORMAT = -4,     /* not a KWAGE database / unsupported compression          */
	KWAGE_ERR_HASH = -5,       /* unknown hash function (reference hash.cpp:92)           */
	KWAGE_ERR_STATE = -6       /* call order violated (e.g. search before finalize)       */
};

/* Limits the reference compiles in (word.h:10, bloom.h:20-21). */
#define KWAGE_MAX_WORD_LEN 32
#define KWAGE_MIN_NUM_HASH 1
#define KWAGE_MAX_NUM_HASH 5
#define KWAGE_HASH_MURMUR32 0      /* hash.h:9 MURMUR_HASH_32 */

/* search flags */
#define KWAGE_SEARCH_EARLY_EXIT 1u /* kwage.cpp:437-483: stop a query tile once no column can
                                      still match. Never changes results, only work done.   */
#define KWAGE_SEARCH_TIMING     2u /* record the HIP-event duration of the gather kernel in the result */
#define KWAGE_SEARCH_TIMING_KMER 4u /* with TIMING: also time the k-mer stage (two more events)         */

const char *kwage_last_error(void);
uint32_t kwage_abi_version(void);

/* ------------------------------------------------------------------------------------
 * Device context
 * ---------------------------------------------------------------------------------- */
typedef struct kwage_ctx kwage_ctx;

/* Number of visible HIP devices (0 if none / no driver). Never fails. */
int kwage_device_count(void);
/* Bind a context to HIP device `device` and create its stream. */
int kwage_init(int device, kwage_ctx **out);
void kwage_shutdown(kwage_ctx *ctx);
/* Free / total device memory in bytes. */
int kwage_mem_info(kwage_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/* Identity of the device behind a context, as one line of `key=value` pairs separated by `;` -- `uuid` (hipDeviceGetUuid,
 * hex), `name`, `arch`, `cus`, `sclk_mhz`, `mclk_mhz`, `hbm_bus_bits`, `pci` (domain:bus:device) -- written NUL-terminated
 * into `buf` (at most `len` bytes; 256 is enough).  The boxes of a pool differ by several per cent in what their HBM
 * delivers: every measurement this repo files carries the line, so two of them can be paired or told apart. */
int kwage_device_fingerprint(kwage_ctx *ctx, char *buf, uint64_t len);
/* Block until everything queued on the context's stream has finished. */
int kwage_sync(kwage_ctx *ctx);

/* Kernel-selection knobs of a context ("walk", "walk_waves", "force_segs", "count_walk", "and_vec", ...: the table in
 * kwage_amd/csrc/engine.hip).  Their values are read ONCE, when the context is created, from the environment
 * (KWAGE_<NAME IN CAPITALS>); afterwards only these calls change them -- nothing on the search path looks at the
 * environment.  For tests and tuning tools: no knob changes any result.  Not while a search is pending. */
int kwage_ctx_set_tuning(kwage_ctx *ctx, const char *name, int64_t value);
int kwage_ctx_get_tuning(kwage_ctx *ctx, const char *name, int64_t *value);
/* Diagnostic: the persistent gather kernels (and_walk_kernel, and_band_walk_kernel, count_walk_kernel) finish the (query,
 * tile) pairs their wave shares cut through small exchange buffers in HBM that they must leave ALL ZERO -- they are
 * cleared when allocated, never per search.  Counts the non-zero 32-bit words of both search slots' buffers:
 * out[0] cut-pair masks, out[1] cut-pair counts + flags (and_walk), out[2] per-query masks, out[3] per-query flags
 * (and_band_walk), out[4] tree arrival counters (count_walk).  Waits for the context's streams first.  tools/soak_walk.py. */
int kwage_ctx_scratch_nonzero(kwage_ctx *ctx, uint64_t out[5]);
/* Diagnostic: what the LAST early-exit search of each slot handed over from its screen launch to its refine launch
 * (kernels.hpp and_screen_kernel / count_screen_kernel): per slot k, out[4k + 0] cluster places, [1] item places and
 * [2] unit places taken (static parts included, i.e. what the refine / emit launches scanned), [3] the capacity of the
 * unit list.  Waits for the context's streams first.  tools/step_breakdown.py, tests. */
int kwage_ctx_refine_stats(kwage_ctx *ctx, uint64_t out[8]);

/* ------------------------------------------------------------------------------------
 * Database group: all columns (samples) that share (kmer_len, num_hash, log_2_filter_len,
 * hash_func), concatenated into ONE wide row-major bit matrix resident in HBM.
 * Replaces the per-file `seekg + slice.read` of kwage.cpp:414-416 / :447-449.
 * Row r, global column c  <->  byte r*row_stride + c/8, bit c%8 (LSB first, bloom.h:143,162).
 * ---------------------------------------------------------------------------------- */
typedef struct kwage_group kwage_group;

typedef struct {
	uint32_t kmer_len;          /* 1..32                    (DBFileHeader::kmer_len)         */
	uint32_t num_hash;          /* 1..5                     (DBFileHeader::num_hash)         */
	uint32_t log_2_filter_len;  /* rows = 1 << this, <= 32  (DBFileHeader::log_2_filter_len) */
	int32_t  hash_func;         /* KWAGE_HASH_MURMUR32      (DBFileHeader::hash_func)        */
} kwage_params;

/* Allocate a group able to hold `column_capacity` columns (rounded up internally so that the
 * row stride is a multiple of 128 bytes). Rows are zero-initialised. */
int kwage_group_create(kwage_ctx *ctx, const kwage_params *params, uint64_t column_capacity,
                       kwage_group **out);
void kwage_group_destroy(kwage_group *g);

/* A SPARSE group: the resident matrix holds only the slices `rows[0..n_rows)` (strictly ascending row indices below
 * 2^log_2_filter_len) of every file added to it -- for a few queries against a database far larger than what they
 * address.  The reference reads only the addressed slices too (one seekg + read per k-mer and hash,
 * kwage.cpp:414-416); here the distinct addressed slices of a whole batch are fetched once per file (host threads,
 * I/O proportional to the queries, not to the database), and searches translate row indices to positions in the
 * list on the device.  Get the rows of a batch from kwage_hash_batch (sort + unique them); searching a batch that
 * addresses a row outside the list fails with KWAGE_ERR_STATE.  kwage_group_add_columns takes images of n_rows rows
 * for such a group; hits, columns and everything else are as for a full group. */
int kwage_group_create_sparse(kwage_ctx *ctx, const kwage_params *params, uint64_t column_capacity,
                              const uint32_t *rows, uint64_t n_rows, kwage_group **out);

/* Append `num_filter` columns from a host image of a file's bit-slice block
 * (2^L rows of ceil(num_filter/8) bytes, `host_row_stride` bytes apart).  The block is placed at
 * the next byte-aligned column; *first_column receives the global index of its column 0. */
int kwage_group_add_columns(kwage_group *g, const void *host_rows, uint64_t host_row_stride,
                            uint32_t num_filter, uint64_t *first_column);

/* Append every column of a NO_COMPRESSION `.db` file (header kwage.h:30-72; body
 * build_db.cpp:243-315), streaming the slice block to the device through pinned staging
 * buffers.  The file's parameters must equal the group's. */
int kwage_group_add_db_file(kwage_group *g, const char *path, uint64_t *first_column,
                            uint32_t *num_filter);

/* The same for `n` files, columns in the order given; first_columns / num_filters (n entries each, may be
 * NULL) receive what kwage_group_add_db_file reports per file.  Prefer this when a group has many files: raw
 * files go file by file through ONE copy-engine pipeline that stays busy across file boundaries (windows of a
 * file are locked in the page cache, copied by SDMA into staging buffers and scattered into the matrix while the
 * next window is being locked: 45-54 GB/s).  Opt-in alternative, KWAGE_LOAD_DIRECT=1: no staging, up to 16 raw
 * files at a time copied side by side by one kernel -- measured slower on a 105 GB matrix of 392 files. */
int kwage_group_add_db_files(kwage_group *g, const char *const *paths, uint32_t n, uint64_t *first_columns,
                             uint32_t *num_filters);

/* Loading progress: while files are loaded through `ctx`, the library adds the bytes of every database file it has
 * passed (whole files, in the order they were given) to *bytes_passed.  The word may lie in memory shared with another
 * process: the CLI's page-cache reader, a child forked before the GPU is touched, keeps a bounded distance ahead of it
 * when the files are not in the page cache.  NULL switches the reporting off (the default). */
void kwage_set_load_progress(kwage_ctx *ctx, volatile uint64_t *bytes_passed);

/* Append `num_columns` synthetic columns: i.i.d. Bernoulli(density_q8/256) bits from a
 * counter-based generator keyed by (seed, row, 64-bit word index) -- generated ON the device. */
int kwage_group_add_random_columns(kwage_group *g, uint64_t num_columns, uint64_t seed,
                                   uint32_t density_q8, uint64_t *first_column);

/* Set individual bits (planting known positives into a synthetic database).  Any column below the span is accepted, a
 * pad or retired column too: every reader masks those by the valid mask, so such bits change no result.  Bits planted in
 * the (up to seven) pad columns between an open tail and the span stay in memory until the next live insert, which
 * continues at the tail, overwrites them -- a kwage_group_compact with nothing to close does not clear them.  The bit
 * densities a finalized group plans its early exit with are NOT re-sampled (planning inputs: they change no result). */
int kwage_group_set_bits(kwage_group *g, const uint32_t *rows, const uint64_t *columns, uint64_t n);

/* Copy `n` whole rows (row_bytes() bytes each) back to the host, `out_stride` bytes apart. */
int kwage_group_read_rows(kwage_group *g, const uint32_t *rows, uint64_t n, void *out,
                          uint64_t out_stride);

/* No more columns will be added; uploads the valid-column mask. Required before searching. */
int kwage_group_finalize(kwage_group *g);

uint64_t kwage_group_num_columns(const kwage_group *g);   /* valid columns added so far       */
uint64_t kwage_group_column_span(const kwage_group *g);   /* next free global column index    */
uint64_t kwage_group_row_bytes(const kwage_group *g);     /* ceil(column_span/8)              */
uint64_t kwage_group_row_stride(const kwage_group *g);    /* bytes between rows in HBM        */
uint64_t kwage_group_device_bytes(const kwage_group *g);  /* HBM held by the bit matrix       */
int kwage_group_params(const kwage_group *g, kwage_params *out);
/* How the matrix's device block was chosen.  Where a large block lies in HBM decides a few per cent of the gather
 * kernels' rate, so where the device has room for two candidate blocks at once, both are allocated, a few milliseconds
 * of the gather pattern are timed on each and the faster one is kept (matrices of 4 GiB and more; context knobs
 * "group_placement_probe" = 0: no second candidate -- releasing the other block costs seconds per 100 GB while the
 * driver wipes it, so one-shot programs turn it off; "group_contiguous" = 0: plain hipMalloc blocks instead of
 * physically contiguous ones; kwage_ctx_set_tuning, or KWAGE_GROUP_PLACEMENT_PROBE / KWAGE_GROUP_CONTIGUOUS in the
 * environment when the context is created).  candidates = blocks compared (1: no choice was made); *_gbps = the probe's rate on the
 * block kept and on the one released (0 with one candidate); windowed_gbps = the probe on the block kept with all waves
 * reading from the same quarter of it at a time -- where that is more than 3 % faster the block mixes regions of the
 * device's memory and the t = 1 walk kernel takes its rows band after band of the matrix (knob "walk_bands" = -1).
 * Any pointer may be NULL. */
int kwage_group_placement(const kwage_group *g, uint32_t *candidates, double *kept_gbps, double *other_gbps, double *windowed_gbps);

/* Live insert, no counterpart in the reference: n whole Bloom filters (filter-major, 2^L bits each, LSB first -- the
 * payload of a `.bloom` file, what kwage_bloom_bits_from_batch writes, the layout kwage_filterset_from_bits reads;
 * for L < 3 a filter is the low 2^L bits of its first byte) become n new columns of the group, transposed on the
 * device.  Allowed before AND after kwage_group_finalize; a finalized group stays finalized and every search
 * submitted after the call returns sees the new columns.  Columns already in the group keep their numbers and bits.
 *   - filter i of the call becomes global column *first_column + i: the columns of one call are contiguous;
 *   - inserts pack densely at BIT granularity.  If the group's last reservation was an insert, the call continues at the
 *     very next column; otherwise (the first insert, or a file, host or random block was added since) it starts at the
 *     next 16-byte boundary of the row, like every other block.  So 1000 filters inserted one at a time take the same
 *     125 bytes of a row as one call of 1000, and the matrix is bit for bit what kwage_group_add_columns makes of the
 *     transposed image.  Every other add closes the open tail (and stays refused after finalize);
 *   - kwage_group_column_span stays a multiple of 8: 8 * ceil(tail / 8), row_bytes = ceil(tail / 8);
 *   - in every row the call owns everything from *first_column to the end of the last 32-bit word it touches (nothing
 *     valid lies above a group's tail): bits of the first word below *first_column % 32 are kept from memory, bits at and
 *     above the new tail are written as zero.  One thread owns a (row, word): no atomics, no read-modify-write outside
 *     that first word;
 *   - afterwards the valid mask, the span and the column count include the new columns, and the bit densities a
 *     finalized group plans its early exit with are re-sampled (planning inputs: they change no result);
 *   - flags: KWAGE_SEARCH_TIMING fills *insert_kernel_ms (may be NULL) with the HIP-event duration of the insert
 *     kernels; other bits are ignored.
 * The host form reads filter i at bits + i*filter_stride_bytes (the stride is ignored when n < 2) and stages chunks of
 * rows through the context's load buffers; the device form reads device memory in place; the third form takes n `.bloom`
 * files, columns in the order given, validated as kwage_build_db validates its inputs -- all n before anything is written.
 * Errors, all found before anything is written -- the span, column count, valid mask and matrix are then as before:
 * KWAGE_ERR_ARG for a NULL argument, n == 0, a sparse group, a host filter_stride_bytes smaller than a filter with
 * n > 1, a device pointer or stride that is not a multiple of 4, or more columns than the group's capacity holds
 * (*first_column + n > 8 * row_stride); KWAGE_ERR_STATE while a search is pending on the context (between
 * kwage_search_submit and its collect); for `.bloom` files KWAGE_ERR_IO (unreadable), KWAGE_ERR_FORMAT (truncated,
 * incomplete, wrong CRC32) or KWAGE_ERR_ARG (kmer_len, num_hash, log_2_filter_len or hash_func differ from the group's).
 * Synchronous; runs on the context's first stream. */
int kwage_group_insert_filters(kwage_group *g, const void *bits, uint64_t filter_stride_bytes, uint32_t n,
                               uint32_t flags, uint64_t *first_column, float *insert_kernel_ms);
int kwage_group_insert_filters_device(kwage_group *g, const void *bits_dev, uint64_t filter_stride_bytes, uint32_t n,
                                      uint32_t flags, uint64_t *first_column, float *insert_kernel_ms);
int kwage_group_insert_bloom_files(kwage_group *g, const char *const *paths, uint32_t n, uint32_t flags,
                                   uint64_t *first_column, float *insert_kernel_ms);
/* Withdraw columns: from the call's return on they are pad columns in every sense -- never reported by any search form,
 * 0 in score, presence and kwage_group_column_bits output, refused by kwage_filterset_from_columns, zeros in
 * kwage_group_read_rows.  Their bits are cleared in every row (the host folds the list into distinct (32-bit word, mask)
 * pairs, one thread per (row, pair)), their valid bits are cleared and the column count drops.  Columns may repeat within
 * a call; groups of either kind, finalized or not.  Retire itself does NOT reuse the space: the span and the numbers of
 * all other columns stay, and a later insert continues at the tail.  kwage_group_compact gives the space back in place
 * (kwage_group_save_db writes the surviving columns densely; a load of that file does it too).  KWAGE_ERR_ARG, nothing changed, for a column at or beyond the span or one
 * that is (already) a pad column; KWAGE_ERR_STATE while a search is pending.  Synchronous. */
int kwage_group_retire_columns(kwage_group *g, const uint64_t *columns, uint64_t n);

/* Compaction, no counterpart in the reference: the gaps that retired columns and the alignment pads of file blocks leave
 * are closed IN PLACE, one pass over the matrix in HBM -- what a save followed by a load also does, without the file and
 * without a second copy of the matrix.  The m valid columns keep their ascending order and become columns 0 .. m - 1;
 * afterwards the matrix is bit for bit what ONE call of the host form of the live insert, given the survivors at
 * column 0, would have made.
 *   - the span becomes 8 * ceil(m / 8), row_bytes = ceil(m / 8); bits m .. span - 1 of every row are zero, and so is
 *     everything from there up to the old span (where the call rewrites rows at all: a group with nothing to close is the
 *     exception, below); the valid mask holds exactly bits [0, m); the column count, the row
 *     stride, the allocation and the row count stay; the tail is open at column m, so the next live insert continues
 *     there at bit granularity and the freed capacity is available at once;
 *   - before and after the finalize call; a finalized group stays finalized and re-samples its bit densities as the live
 *     insert does.  Every search submitted after the call returns sees the new column numbers;
 *   - new_column (may be NULL) receives, for every column c below the OLD span, the column's new number -- the number of
 *     valid columns below c -- or KWAGE_NO_COLUMN for a pad or retired column; capacity is the number of entries the
 *     array holds;
 *   - a destination column never lies above its source, so a row is rewritten left to right in segments of 16-byte
 *     units: a segment's units are all made in registers before any of them is stored (a workgroup barrier between the
 *     two), one 16-byte store per unit, no atomics.  Units wholly below the first pad or retired column are not touched;
 *   - m == 0 is allowed: the span becomes 0 and no kernel is launched.  A group with nothing to close (every column
 *     below the tail valid) launches nothing and returns the identity map; since nothing is written then, bits that
 *     kwage_group_set_bits planted in the pad columns between the open tail and the span (columns m .. span - 1) are
 *     NOT zero afterwards: they stay, masked by the valid mask in every reader, until the next live insert overwrites
 *     everything from column m on;
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the kernel; other bits are
 *     ignored.  stats may be NULL.
 * Errors, all found before a byte is written -- the matrix, valid mask and span are then as before: KWAGE_ERR_ARG for a
 * NULL group, a sparse group, a non-NULL new_column with capacity below the old span; KWAGE_ERR_STATE while a search is
 * pending on the context.  Synchronous; runs on the context's first stream. */
#define KWAGE_NO_COLUMN 0xFFFFFFFFFFFFFFFFull
typedef struct {
	uint64_t span_before, span_after;   /* kwage_group_column_span before / after            */
	uint64_t columns;                   /* valid columns m (unchanged by the call)           */
	uint64_t runs;                      /* stretches of consecutive surviving columns        */
	uint64_t first_unit, units;         /* 16-byte units of a row rewritten: [first_unit, first_unit + units) */
	float    kernel_ms;                 /* with KWAGE_SEARCH_TIMING in flags, else 0         */
} kwage_compact_stats;
int kwage_group_compact(kwage_group *g, uint32_t flags, uint64_t *new_column, uint64_t capacity, kwage_compact_stats *stats);

/* Fold, no counterpart among the reference's programs: a NEW group whose Bloom filters are 2^log_2_filter_len bits long,
 * made on the device from a resident group with longer ones -- rows per sample is the one size knob of the format, and
 * this turns it without rebuilding a `.bloom` file.  The reference takes a row index as hash % filter_len with a
 * power-of-two length (kwage.cpp:411-412, :445), so the filter of a k-mer set at L' = log_2_filter_len is exactly the OR of
 * the 2^(L - L') consecutive pieces of the same set's filter at L with the same num_hash (how make_bloom_filter itself
 * shortens a filter, make_bloom.cpp:344-354); in the bit-sliced matrix: dst row r' = OR over j of src row r' + j * 2^L'.
 *   - *out is a new group on src's context: kmer_len, num_hash and hash_func are src's, log_2_filter_len the argument; row
 *     stride and column capacity are src's; the matrix comes from kwage_group_create's allocation path, zero-initialised,
 *     the placement rule applied as there (kwage_group_placement);
 *   - the column layout is src's, number for number: span, row_bytes, column count, valid mask, and the open tail of a
 *     live insert.  A column keeps its number; retired and pad columns stay what they were, and bits that
 *     kwage_group_set_bits planted in pad columns are folded like any others and stay masked;
 *   - with U = ceil(row_bytes / 16), bytes [0, 16 U) of dst row r' are the OR of the same bytes of src rows
 *     r' + j * 2^L', j < 2^(L - L'); bytes from 16 U to the stride are zero.  One lane makes one 16-byte unit of one
 *     destination row from eight loads in flight and one store: one streaming pass, no atomics;
 *   - src finalized: *out is finalized -- its valid mask uploaded, its bit densities sampled as compact and the live insert
 *     do; src open: *out is open, and further adds and inserts continue exactly where they would have on src;
 *   - src, its matrix, mask and state are not changed;
 *   - 0 <= log_2_filter_len < src's; 0 gives one row;
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the kernel; other bits are
 *     ignored.  stats may be NULL.
 * Errors, all found before anything is allocated, *out not written: KWAGE_ERR_ARG for a NULL src or out, a sparse group,
 * log_2_filter_len at or above src's; KWAGE_ERR_STATE while a search is pending on the context.  An allocation that fails
 * returns kwage_group_create's error with nothing kept.  Synchronous; runs on the context's first stream. */
typedef struct {
	uint32_t log_2_before, log_2_after;
	uint64_t units_per_row;          /* 16-byte units of a row read and written: ceil(row_bytes / 16) */
	uint64_t bytes_read, bytes_written;
	float    kernel_ms;              /* with KWAGE_SEARCH_TIMING in flags, else 0 */
} kwage_fold_stats;
int kwage_group_fold(kwage_group *src, uint32_t log_2_filter_len, uint32_t flags, kwage_group **out, kwage_fold_stats *stats);

/* Copy between groups, no counterpart in the reference: n columns of the resident group src become n new columns of the
 * resident group dst, packed on the device in one pass over the rows -- how a group grows (everything copied into a wider
 * one), how groups that share their parameters merge, how a working subset is split off -- without the two transposes and
 * the host image of kwage_group_export_filters followed by kwage_group_insert_filters.
 *   - columns[i] is a valid column of src and becomes column *first_column + i of dst: the columns of one call are
 *     contiguous in dst, in list order.  columns == NULL with n == 0 means every valid column of src, ascending;
 *   - placement is exactly the live insert's: where dst's last reservation was an insert (or a copy), the call continues at
 *     the very next column at bit granularity; otherwise it starts at the next 16-byte boundary of the row;
 *   - after the call dst is bit for bit in the state kwage_group_insert_filters(dst, <those columns exported from src>)
 *     would have left: the matrix up to the stride, the span, the valid mask, the column count, the open tail, and --
 *     dst finalized -- finalized still, its bit densities re-sampled.  Bits of the first word below *first_column are kept
 *     from memory; bits at and above the new tail are written as zero, to the end of the last 32-bit word the call
 *     touches -- what the insert owns; bits that kwage_group_set_bits planted between an open tail and the span are
 *     overwritten;
 *   - src, its matrix, mask and state are not changed; bits in pad or retired columns of src never travel: a listed
 *     column's neighbours in a source word are masked out;
 *   - one lane makes one 16-byte unit of one destination row and stores it once; dst is read only by the owner of a
 *     row's first unit (where *first_column is no multiple of 128, for the bits below it) and of its last unit (where the
 *     last word written is not the unit's last, for the words above it).  No atomics;
 *   - before and after kwage_group_finalize, on either group, independently;
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the kernel; other bits are
 *     ignored.  stats may be NULL.
 * Errors, all found before a byte is written or allocated -- *first_column and *stats are not written, dst is as before --
 * in this order: KWAGE_ERR_ARG for a NULL dst, src or first_column; columns == NULL with n != 0, or columns != NULL with
 * n == 0; dst == src; groups of different contexts; a sparse group on either side; kmer_len, num_hash, log_2_filter_len
 * or hash_func differing; then KWAGE_ERR_STATE while a search is pending on the context; then KWAGE_ERR_ARG again for a
 * src without valid columns in the all-columns form; n > 2^32 - 1; a column at or beyond src's span, a pad or retired
 * column, a column listed twice (the first offender in list order); more columns than dst's capacity holds
 * (*first_column + n > 8 * row_stride).  Synchronous; runs on the context's first stream. */
typedef struct {
	uint64_t first_column;            /* where columns[0] went in dst                                   */
	uint64_t columns;                 /* n copied                                                       */
	uint64_t runs;                    /* stretches of consecutive source columns the list folded into   */
	uint64_t first_unit, units;       /* 16-byte units of a dst row written: [first_unit, first_unit+units) */
	uint64_t bytes_written;           /* rows * units * 16                                              */
	float    kernel_ms;               /* with KWAGE_SEARCH_TIMING in flags, else 0                      */
} kwage_copy_stats;
int kwage_group_copy_columns(kwage_group *dst, kwage_group *src, const uint64_t *columns, uint64_t n,
                             uint32_t flags, uint64_t *first_column, kwage_copy_stats *stats);

/* Union of columns, no counterpart in the reference: n_sets new columns of the resident group dst, each the row-wise OR
 * of listed columns of the resident group src, made on the device in one pass over the rows.  A row index is
 * hash % filter_len (kwage.cpp:411-412), so the OR of the filters of k-mer sets A and B is the filter of A u B: the new
 * column is byte for byte the filter the reference would have built from the members' reads together -- several runs
 * of one biosample as one sample, one pan-filter of a species' samples -- without kwage_group_export_filters, an OR on the
 * host and kwage_group_insert_filters.
 *   - new column *first_column + j of dst is, in every row, the OR of src's columns
 *     columns[set_offsets[j] .. set_offsets[j + 1]); set_offsets has n_sets + 1 entries and starts at 0.  A member may stand
 *     in several sets; a member repeated within a set is folded; a set of one member is a copy of that column;
 *   - dst != src: placement, the bits written and the state afterwards are kwage_group_copy_columns', hence the live
 *     insert's: behind an open tail at bit granularity, else at the next 16-byte boundary of the row; bits below
 *     *first_column are kept from memory, bits at and above the new tail are written as zero to the end of the last
 *     32-bit word touched; the valid mask, span, open tail and column count follow, and a finalized dst re-samples its
 *     bit densities.  dst is afterwards bit for bit what kwage_group_insert_filters(dst, <the ORs of the members' exported
 *     filters>) would have made of it;
 *   - dst == src is allowed -- a union usually lands in the group that holds its members.  The new columns then start at
 *     the next 16-byte boundary of the row ALSO behind an open tail: the up to 127 columns skipped become pad columns, as
 *     between two file blocks (kwage_group_compact closes them), and the tail is open at *first_column + n_sets
 *     afterwards.  The skipped columns are not written: they hold what the memory held -- zero behind a fresh insert up
 *     to the end of its last 32-bit word, but whatever a compaction that kept the memory (no valid column left) or
 *     kwage_group_set_bits left there beyond it -- and come below the span as dead columns with those bits: no search,
 *     kwage_group_column_bits, fold, compaction, save or export counts them.  Likewise the bits above the last 32-bit
 *     word the union touches are kept, as behind any live insert, and show when the span grows over them.
 *     Members lie in valid columns below the old span and every 16-byte unit written lies wholly above it,
 *     so the kernel never reads a byte it writes: no ordering, fence or atomic is needed.  The cost is the pad: a call
 *     per union wastes up to 127 columns each time -- batch many unions into one call;
 *   - src's own columns are never changed.  Bits that kwage_group_set_bits left in pad or retired columns never travel:
 *     the masks name member bits only;
 *   - the host folds the lists into distinct (source dword of the row, 32-bit mask) pairs per set: members that share a
 *     dword cost one load.  One lane makes one 16-byte unit of one destination row and stores it once; dst is read only by
 *     the owners of a row's first and last unit, for what they keep.  No atomics;
 *   - before and after kwage_group_finalize, on either group;
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the kernel; other bits are
 *     ignored.  stats may be NULL.
 * Errors, all found before a byte is written or allocated -- *first_column and *stats are not written, both groups are as
 * before -- in this order: KWAGE_ERR_ARG for a NULL dst, src, columns, set_offsets or first_column; n_sets == 0;
 * set_offsets[0] != 0, a decreasing offset or an empty set; groups of different contexts; a sparse group on either side;
 * kmer_len, num_hash, log_2_filter_len or hash_func differing; then KWAGE_ERR_STATE while a search is pending on the
 * context; then KWAGE_ERR_ARG again for a member at or beyond src's span, a pad or retired column (the first offender in
 * list order); more than 2^32 - 1 members (or entries); more sets than dst's capacity holds
 * (*first_column + n_sets > 8 * row_stride).  Synchronous; runs on the context's first stream. */
typedef struct {
	uint64_t first_column, sets, members;  /* members: list entries as given                         */
	uint64_t entries;                      /* (source dword, mask) pairs after folding               */
	uint64_t first_unit, units;            /* 16-byte units of a destination row written             */
	uint64_t bytes_written;
	float kernel_ms;                       /* with KWAGE_SEARCH_TIMING, else 0                       */
} kwage_union_stats;
int kwage_group_union_columns(kwage_group *dst, kwage_group *src, const uint64_t *columns, const uint64_t *set_offsets, uint32_t n_sets,
                              uint32_t flags, uint64_t *first_column, kwage_union_stats *stats);

/* Overlap matrix, no counterpart in the reference: for every pair of listed columns of two resident groups the number of
 * rows in which both are set -- with M the rows x columns bit matrix, shared(i, j) = popcount(col_i AND col_j) =
 * (M_a^T M_b)[i][j], formed as that integer matrix product on the matrix cores (v_mfma_i32_32x32x32_i8).  It is what a
 * Jaccard index of two samples is made of, for all pairs at once: its cost does not depend on how full the filters are,
 * it needs no row list (kwage_filterset_from_columns) and only a RESIDENT group, finalized or not.
 *   - cell (i, j) is a uint32 at cells[i*row_elems + j]: the rows in which column cols_a[i] of a and column cols_b[j] of b
 *     are both set.  row_elems >= the cells of a row; cells from there to row_elems are not touched; cells_dev is 4-byte
 *     aligned.  Nothing has to be cleared beforehand;
 *   - the lists are taken as kwage_group_export_filters takes them: any order, a column may be named more than once;
 *   - cols_x == NULL with n_x == 0: every column 0 .. span - 1 of that group.  Pad and retired columns then give a row (or
 *     column) of zeros, as the score matrix does.  Dead columns are taken out with the valid mask: bits that
 *     kwage_group_set_bits or a file's pad left in them never count;
 *   - b == NULL with cols_b == NULL and n_b == 0 is the SYMMETRIC form, a's list against itself: only the tiles (128 x 128
 *     cells) on or above the diagonal are computed and the others are written as their mirror, so the result is symmetric
 *     by construction; its diagonal is kwage_group_column_bits;
 *   - b != NULL: b may be a itself or another resident group of the same context with the same kmer_len, num_hash,
 *     log_2_filter_len and hash_func; the row strides may differ;
 *   - the lists are cut into blocks of 32 columns: a block of 32 consecutive columns that starts at a multiple of 32 is
 *     STRAIGHT (one dword of a row feeds it), any other is GATHERED column by column.  Where the tiles are fewer than the
 *     device needs, the row range is cut into `splits` parts whose partial tiles (a block of the context's pool) a second
 *     kernel sums: integer sums, exact in any order, so the cells do not depend on the split (knob "overlap_splits").
 *     Every cell is stored once by one lane; no atomics; no floating point;
 *   - before and after kwage_group_finalize; both groups are only read;
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the kernels; other bits are
 *     ignored.  stats may be NULL.
 * The host form computes the cells in a block of the context's pool and copies them out with one strided copy.
 * Errors, all found before a kernel runs or a byte is allocated -- cells and *stats are not written -- in this order:
 * KWAGE_ERR_ARG for a NULL a or cells; a NULL list with a nonzero count or a list with a zero count (a's, then b's); a
 * NULL b with cols_b; groups of different contexts; a sparse group on either side; kmer_len, num_hash, log_2_filter_len
 * or hash_func differing; log_2_filter_len == 32 (a count of 2^32 does not fit a cell); row_elems smaller than the cells of
 * a row; then KWAGE_ERR_STATE while a search is pending on the context; then KWAGE_ERR_ARG again for a listed column at or
 * beyond its group's span or a pad or retired column (the first offender in list order, a's list before b's); a launch
 * that does not fit a grid; then the pool's error (KWAGE_ERR_DEVICE), with the number of bytes needed, where the tables,
 * the partial sums or the host form's block cannot be had.  An empty group with NULL lists writes nothing and succeeds.
 * Synchronous; runs on the context's first stream. */
typedef struct {
	uint64_t n_a, n_b, rows;          /* cells are n_a x n_b, summed over rows = 2^L            */
	uint64_t tiles, splits;           /* workgroup tiles computed; parts the row range was cut in */
	uint64_t straight_blocks, gathered_blocks;   /* 32-column blocks of either kind               */
	uint32_t symmetric;               /* 1: only tiles on or above the diagonal were computed   */
	float kernel_ms;                  /* with KWAGE_SEARCH_TIMING, else 0                       */
} kwage_overlap_stats;
int kwage_group_column_overlaps_device(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                       void *cells_dev, uint64_t row_elems, uint32_t flags, kwage_overlap_stats *stats);
int kwage_group_column_overlaps(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                uint32_t *cells, uint64_t row_elems, uint32_t flags, kwage_overlap_stats *stats);
/* Which kernels the calling thread's last overlap call launched: "overlap_mfma_kernel" or
 * "overlap_mfma_kernel+overlap_combine_kernel"; "" if none.  Valid until the thread's next one. */
const char *kwage_group_overlap_kernel(void);

/* Nearest-neighbour lists, no counterpart in the reference: for every listed column of a its k best partners among the
 * listed columns of b, chosen ON THE DEVICE from the overlap matrix's cells.  The cells are computed strip by strip of
 * a's list by the overlap kernels into one block of the context's pool and discarded as soon as a strip's rows have been
 * reduced to k records each: what leaves the device is n_a x k records of 16 bytes, never n_a x n_b cells.
 *   - lists and groups exactly as kwage_group_column_overlaps takes them: any order, repeats allowed, NULL with count 0 =
 *     every column of the span, b == NULL = a's list is also the candidate list, b may be a or another group of the
 *     context with the same parameters; before and after finalize; both groups are only read;
 *   - candidate j (place j of b's list; column j under a NULL list) is ELIGIBLE for entry i of a's list iff its column is
 *     live (valid mask), entry i's column is live, shared(i, j) >= min_shared, and -- with KWAGE_NEIGHBORS_SKIP_SELF in
 *     flags and b NULL or == a -- it does not name the same COLUMN as entry i (every repeat of that column among the
 *     candidates is skipped; with another group as b the flag has no effect);
 *   - a record is {index = j, shared = the overlap cell, bits_a, bits_b = the set bits of the two columns
 *     (kwage_group_column_bits' values)};
 *   - order: key descending, then index ascending, EXACT.  KWAGE_NEIGHBORS_SHARED: key = shared.
 *     KWAGE_NEIGHBORS_JACCARD: the order of the fractions shared / (bits_a + bits_b - shared) -- s1 u2 > s2 u1 in 64-bit
 *     integers -- with an empty union counting as 0; never a float.  (On the device the scalar key is
 *     floor(shared 2^64 / union), all ones where shared == union: two distinct fractions with denominators <= 2^32 differ
 *     by at least 2^-64, so it is strictly monotone in the fraction.);
 *   - counts[i] = min(k, eligible candidates of entry i); out[i*k + r], r < counts[i], is the r-th best record; every
 *     record with r >= counts[i] is {0xFFFFFFFF, 0, 0, 0}.  All n_a x k records and n_a counts are written, each once;
 *     nothing has to be cleared beforehand, nothing else is touched.  out_dev and counts_dev are 4-byte aligned;
 *   - 1 <= k <= KWAGE_TOPK_MAX;
 *   - a's list is cut into STRIPS of strip_entries entries: the largest multiple of 128 whose cells -- a row of cells is
 *     the candidates rounded up to a multiple of 4 -- fit the knob "neighbors_strip_bytes" (default 256 MiB), at least 128
 *     and at most n_a.  Per strip the overlap kernels run in the a x b form (the symmetric saving is not used), then
 *     neighbors_select_kernel: one workgroup per entry, an 8-bit radix select over (key, index) with histograms in LDS,
 *     the winners ordered by a bitonic sort.  No global atomics, no floating point.  The result does not depend on the
 *     strips or on "overlap_splits";
 *   - flags: KWAGE_SEARCH_TIMING fills stats->kernel_ms with the HIP-event duration of the overlap and select kernels of
 *     all strips; KWAGE_NEIGHBORS_SKIP_SELF; other bits are ignored.  stats may be NULL.
 * The host form writes to blocks of the pool and copies records and counts out.
 * Errors, all found before a kernel runs or a byte is allocated -- out, counts and *stats are not written -- in this
 * order: KWAGE_ERR_ARG for a NULL a, out or counts; k out of range; an unknown metric; then every refusal of
 * kwage_group_column_overlaps from "a NULL list with a nonzero count" on, in its order and wording (there is no row_elems);
 * then the pool's error (KWAGE_ERR_DEVICE) with the bytes asked for.  An empty a-list (an empty group with a NULL list)
 * writes nothing and succeeds; an empty candidate side gives counts of 0 and filler records.
 * Synchronous; runs on the context's first stream. */
#define KWAGE_NEIGHBORS_SHARED   0u   /* key = shared */
#define KWAGE_NEIGHBORS_JACCARD  1u   /* key = shared / (bits_a + bits_b - shared), 0 where that union is empty */
#define KWAGE_NEIGHBORS_SKIP_SELF 0x100u   /* in flags */
typedef struct { uint32_t index, shared, bits_a, bits_b; } kwage_neighbor;   /* 16 bytes */
typedef struct {
	uint64_t n_a, n_b, rows;
	uint64_t strips, strip_entries;   /* strips of a's list; entries of a full strip (a multiple of 128, or n_a) */
	uint64_t tiles;                   /* overlap tiles computed, all strips together */
	uint64_t records;                 /* sum of counts */
	uint32_t metric;
	float kernel_ms;                  /* with KWAGE_SEARCH_TIMING: overlap + select kernels of all strips, else 0 */
} kwage_neighbors_stats;              /* 64 bytes */
int kwage_group_column_neighbors_device(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                        uint32_t k, uint32_t metric, uint32_t min_shared, void *out_dev, void *counts_dev, uint32_t flags,
                                        kwage_neighbors_stats *stats);
int kwage_group_column_neighbors(kwage_group *a, const uint64_t *cols_a, uint32_t n_a, kwage_group *b, const uint64_t *cols_b, uint32_t n_b,
                                 uint32_t k, uint32_t metric, uint32_t min_shared, kwage_neighbor *out, uint32_t *counts, uint32_t flags,
                                 kwage_neighbors_stats *stats);
/* The kernels of the strips the calling thread's last neighbours call launched -- the stages KWAGE_SEARCH_TIMING times:
 * "overlap_mfma_kernel+neighbors_select_kernel", "overlap_mfma_kernel+overlap_combine_kernel+neighbors_select_kernel" where
 * a strip's row range was cut into parts, "neighbors_select_kernel" alone where the candidate side is empty; "" if none.
 * The string does not name neighbors_bits_kernel and neighbors_bits_sum_kernel, which every call with a non-empty a-list
 * runs once beforehand, outside the timed section: they count the set bits of EVERY column of either group's span,
 * however few are listed (kwage_group_column_bits_device refuses a group that is not finalized; this call does not).
 * Valid until the thread's next one. */
const char *kwage_group_neighbors_kernel(void);

/* ------------------------------------------------------------------------------------
 * Query batch: raw sequences (any case, any characters -- exactly what the reference hands to
 * search(), kwage.cpp:119,137), concatenated, uploaded once and kept resident in HBM.
 * ---------------------------------------------------------------------------------- */
typedef struct kwage_batch kwage_batch;

/* `offsets` has n_queries+1 entries; query i is bytes [offsets[i], offsets[i+1]) of `seqs`. */
int kwage_batch_create(kwage_ctx *ctx, const char *seqs, const uint64_t *offsets,
                       uint32_t n_queries, kwage_batch **out);
void kwage_batch_destroy(kwage_batch *b);
uint32_t kwage_batch_num_queries(const kwage_batch *b);

/* ------------------------------------------------------------------------------------
 * Search: for every query of the batch against every column of the group, what
 * search() computes (kwage.cpp:340-541): canonical k-mer set, MurmurHash3 row indices,
 * row gather + AND (threshold == 1.0f) or per-column counts (threshold < 1), hit extraction.
 * ---------------------------------------------------------------------------------- */
typedef struct {
	uint32_t query;      /* index into the batch                                            */
	uint32_t column;     /* global column of the group                                      */
	uint32_t num_match;  /* MatchResult::num_kmers_found (kwage.cpp:517-518)                */
} kwage_hit;

typedef struct {
	uint64_t n_hits;
	const kwage_hit *hits;          /* sorted by (query, column)                              */
	uint32_t n_queries;
	const uint32_t *num_query_kmer; /* per query: distinct canonical k-mers (kwage.cpp:366)   */
	const uint32_t *query_threshold;/* per query: (unsigned)(float t * n) (kwage.cpp:388); 0 at t==1 */
	uint64_t total_kmers;           /* sum of num_query_kmer                                  */
	uint64_t bit_tests;             /* total_kmers * num_hash * num_columns                   */
	uint64_t algorithmic_bytes;     /* total_kmers * num_hash * ceil(num_columns/8)           */
	float kmer_kernel_ms;           /* with KWAGE_SEARCH_TIMING, else 0                       */
	float search_kernel_ms;         /* the gather + AND / count kernel                        */
	uint32_t search_kernel_launches;/* >1 if the hit buffer had to grow and the kernel re-ran */
	const char *search_kernel;      /* which gather kernel ran, with its template shape: "and_kernel<2,8,nt>",
	                                 * "and_walk_kernel<13,4>", "and_narrow_kernel<4,8>", "count_kernel<10,5>",
	                                 * "count_narrow_kernel<7,1,4>", "...+segments"; "" if none.  Owned by the result. */
} kwage_result;

/* Order `n` hit records by (query, column) in place, on the host (LSD radix sort on the 64-bit key; no device is
 * touched).  What a caller that gathers the unsorted device-resident lists of several shards needs after adding each
 * shard's column base (kwage_amd/distributed.py). */
void kwage_sort_hits(kwage_hit *hits, uint64_t n);

int kwage_search(kwage_group *g, kwage_batch *b, float threshold, uint32_t flags,
                 kwage_result **out);
void kwage_result_free(kwage_result *r);

/* Top-k search, with no counterpart in the reference: for every query, the k best-scoring columns of the group.
 *   - a column's score is its num_match: what kwage_search reports for it at a threshold whose floor is f below;
 *   - per query with n distinct k-mers the floor is f = kwage_query_threshold(threshold, n); eligible are the real
 *     columns with score >= f (pad bits never count); threshold 0 means "the k best, whatever their score";
 *   - the selection is the first min(k, #eligible) eligible columns under the key (score descending, column
 *     ascending); across files or groups a host merges under (score descending, file order, column ascending);
 *   - a query without k-mers (n = 0) has no hits;
 *   - 1 <= k <= KWAGE_TOPK_MAX and 0 <= threshold <= 1, else KWAGE_ERR_ARG.
 * The result is a kwage_result, freed with kwage_result_free; its records are ordered by (query, column) like every
 * other result, query_threshold = the floor f (n at threshold 1), search_kernel names the kernels that ran,
 * KWAGE_SEARCH_TIMING / _TIMING_KMER are honoured.  KWAGE_SEARCH_EARLY_EXIT is ignored: every tile is counted to
 * the end (no exact bound is kept across tiles).  Synchronous; runs on the context's first stream. */
#define KWAGE_TOPK_MAX 1024u
int kwage_search_topk(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags,
                      kwage_result **out);

/* The top-k search with its records left on the device, for hosts that merge the lists of several groups, shards or
 * passes themselves (kwage_node's top-k form): kwage_search_topk is to this what kwage_search is to
 * kwage_search_device_append_submit.  The same records as kwage_search_topk selects, `column_base` added to every
 * column, appended behind the *count_dev records already in hits_dev (count_dev: a device uint64, required;
 * reset_count != 0 zeroes it first).  Records go query by query, each query's by column; records beyond `capacity` are
 * counted, not stored (grow the buffer and redo the list).  num_query_kmer_dev may be NULL or a device buffer of
 * n_queries uint32.  Synchronous, on the context's first stream: *n_total receives the running total, which is also
 * in *count_dev when the call returns.  Timing flags are ignored.  Errors as kwage_search_topk, and KWAGE_ERR_ARG when
 * column_base + the group's column span exceeds 32 bits. */
int kwage_search_topk_device_append(kwage_group *g, kwage_batch *b, uint32_t k, float threshold, uint32_t flags,
                                    void *hits_dev, uint64_t capacity, void *count_dev, uint32_t column_base,
                                    int reset_count, void *num_query_kmer_dev, uint64_t *n_total);

/* Device merge of top-k lists: hits_dev holds n_hits kwage_hit records (several lists concatenated, in any order).
 * out_dev receives, per query, the first min(k, #records of the query) records under the key (num_match descending,
 * order[column] ascending), ordered by (query, column) like every result; the output does not depend on the order of
 * the input.  order_dev is a device array of n_order uint32 tie keys indexed by column (file order then column, for
 * lists whose global columns are not in file order), or NULL: the tie key is the column itself.
 * *out_count_dev (a device uint64, required) receives the output's record count.
 * Preconditions, NOT checked: a (query, column) pair appears at most once; order is injective on the columns present.
 * Errors (KWAGE_ERR_ARG): k = 0 or k > KWAGE_TOPK_MAX; a NULL ctx or out_count_dev, NULL hits_dev with n_hits > 0,
 * NULL out_dev with out_capacity > 0; n_hits >= 2^32 or n_queries >= 2^31; records whose query is >= n_queries or,
 * with an order table, whose column is >= n_order (found on the device, ignored by the merge, reported after it); an
 * output larger than out_capacity (the first out_capacity records are written, *out_count_dev holds the full count).
 * Synchronous; runs on the context's first stream; device scratch comes from the context's pool. */
int kwage_topk_merge_device(kwage_ctx *ctx, const void *hits_dev, uint64_t n_hits, uint32_t n_queries, uint32_t k,
                            const void *order_dev, uint64_t n_order, void *out_dev, uint64_t out_capacity,
                            void *out_count_dev);

/* Dense score search, no counterpart in the reference: cell (q, c) = the num_match kwage_search would report for
 * column c and query q at a threshold whose floor is 0; 0 for pad columns (never counted) and for a query without k-mers.
 *   - cells are uint32; cell (q, c) lies at scores[q*row_elems + c] for c in [0, kwage_group_column_span(g)); cells at
 *     or beyond the span in a row are not touched;
 *   - row_elems >= the span and row_elems % 4 == 0; scores_dev is 16-byte aligned.  Spans and the column bases of
 *     groups are multiples of 8 columns, so a caller places several groups side by side in one matrix by offsetting
 *     the pointer;
 *   - num_query_kmer / num_query_kmer_dev may be NULL or hold n_queries uint32 (host / device memory);
 *   - KWAGE_SEARCH_TIMING fills *search_kernel_ms (may be NULL) with the HIP-event duration of the score kernels;
 *     KWAGE_SEARCH_EARLY_EXIT is ignored: every column is counted to the end.
 * Errors of two kinds.  Found on the host before any kernel is launched: KWAGE_ERR_STATE before kwage_group_finalize;
 * KWAGE_ERR_ARG for mixed contexts, a wrong row_elems, a misaligned or NULL pointer, a query of 2^32 rows and more, or
 * a batch too large for one launch.  Found on the device: KWAGE_ERR_STATE for a sparse group whose row list does not
 * cover the batch, which is known only once the k-mer stage has computed the batch's rows; a search of a sparse group
 * waits for that answer (one 8-byte copy) before it launches the score kernels, so in either kind no cell is written.
 * Synchronous; runs on the context's first stream; device scratch comes from the context's pool.  kwage_search_scores
 * is the same search with the matrix copied to host memory. */
int kwage_search_scores_device(kwage_group *g, kwage_batch *b, void *scores_dev, uint64_t row_elems,
                               void *num_query_kmer_dev, uint32_t flags, float *search_kernel_ms);
int kwage_search_scores(kwage_group *g, kwage_batch *b, uint32_t *scores, uint64_t row_elems,
                        uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms);
/* Which kernels the calling thread's last dense score search launched, with their template shapes:
 * "score_tile_kernel<10,1>", "count_kernel<7,1>+score_combine_kernel<14>"; "" if none.  Valid until the thread's next one. */
const char *kwage_search_scores_kernel(void);

/* Presence search, no counterpart in the reference: one pass/fail bit per (query, column), the matrix a BIGSI-style
 * index answers with.  Query q has n distinct k-mers and the floor f = kwage_query_threshold(threshold, n) (n at t = 1);
 * bit (q, c) is 1 iff n > 0, c is a real column and the column's num_match >= f: exactly the (q, c) for which
 * kwage_search(g, b, threshold, ...) returns a record, for every 0 < t <= 1 and n < 2^24.  With floor 0 every real
 * column of a query that has k-mers passes.  Pad bits are 0; the row of a query without k-mers is 0.
 *   - bit (q, c) lies at bits[q*row_bytes + c/8], bit c%8 (LSB first): the layout of a row of the resident matrix;
 *   - with W = kwage_group_row_bytes(g) rounded up to 16: row_bytes >= W and row_bytes % 16 == 0; bits_dev is 16-byte
 *     aligned.  Bytes [0, W) of every row are written (nothing has to be cleared beforehand), bytes at or beyond W
 *     are not touched;
 *   - passing / passing_dev may be NULL or receive n_queries uint32: the set bits of each query's row;
 *   - num_query_kmer / num_query_kmer_dev may be NULL or hold n_queries uint32 (host / device memory);
 *   - KWAGE_SEARCH_TIMING fills *search_kernel_ms (may be NULL) with the HIP-event duration of the presence kernels;
 *     KWAGE_SEARCH_EARLY_EXIT lets a (query, KiB tile) in which no column can pass any more stop and store its zeros:
 *     the bitmap is bit for bit the same with and without it (the segmented form of few long queries ignores it).
 * Errors of two kinds.  Found on the host before any kernel is launched: KWAGE_ERR_STATE before kwage_group_finalize;
 * KWAGE_ERR_ARG for mixed contexts, a wrong row_bytes, a misaligned or NULL pointer, a threshold outside [0, 1] (NaN
 * included), a query of 2^32 rows and more, or a batch too large for one launch.  Found on the device: KWAGE_ERR_STATE
 * for a sparse group whose row list does not cover the batch, known once the k-mer stage has computed the batch's rows
 * and before the first presence kernel.  In either kind nothing of the caller's memory is written.
 * Synchronous; runs on the context's first stream; device scratch comes from the context's pool.
 * kwage_search_presence is the same search with the bitmap copied to host memory. */
int kwage_search_presence_device(kwage_group *g, kwage_batch *b, float threshold, void *bits_dev, uint64_t row_bytes,
                                 void *passing_dev, void *num_query_kmer_dev, uint32_t flags, float *search_kernel_ms);
int kwage_search_presence(kwage_group *g, kwage_batch *b, float threshold, uint8_t *bits, uint64_t row_bytes,
                          uint32_t *passing, uint32_t *num_query_kmer, uint32_t flags, float *search_kernel_ms);
/* Which kernels the calling thread's last presence search launched, with their template shapes:
 * "presence_tile_kernel<10,1>", "count_kernel<7,1>+presence_combine_kernel<14>", "presence_and_kernel"; "" if none.
 * Valid until the thread's next one. */
const char *kwage_search_presence_kernel(void);

/* Filter set, no counterpart in the reference: n whole Bloom filters over 2^L rows as the QUESTIONS of a search ("which
 * samples look like this sample").  On the device a set is one concatenated uint32 row list -- the rows in which each
 * filter is set, ascending -- with a uint64 prefix array of n + 1 entries and each filter's set-bit count: the shape a
 * batch's row indices have after the k-mer stage.  A set belongs to its context and carries the kwage_params it was
 * made with; its device memory comes from and returns to the context's pool, so it is destroyed before the context.
 *   - from_columns: `columns` are global column numbers of a finalized, non-sparse group (the same column may be named
 *     twice).  KWAGE_ERR_STATE before kwage_group_finalize; KWAGE_ERR_ARG for a column at or beyond the span, a pad
 *     column, a sparse group.
 *   - from_bits: `bits` holds n host bit vectors of 2^L bits each, LSB first (the payload order of a `.bloom` file,
 *     what kwage_bloom_bits_from_batch writes), filter_stride_bytes apart (ignored when n < 2).  For L < 3 a filter
 *     is the low 2^L bits of one byte; higher bits are ignored.
 *   - both: L = 32 is refused (KWAGE_ERR_ARG: a full filter's count does not fit 32 bits), as is a set too large for
 *     one launch; n = 0 gives a valid empty set; a row list that cannot be allocated returns the pool's error.  On
 *     any error *out is not written.
 * Synchronous; runs on the context's first stream. */
typedef struct kwage_filterset kwage_filterset;
int kwage_filterset_from_columns(kwage_group *g, const uint64_t *columns, uint32_t n, kwage_filterset **out);
int kwage_filterset_from_bits(kwage_ctx *ctx, const kwage_params *params, const void *bits, uint64_t filter_stride_bytes,
                              uint32_t n, kwage_filterset **out);
void kwage_filterset_destroy(kwage_filterset *fs);
uint32_t kwage_filterset_num_filters(const kwage_filterset *fs);
/* Every filter's set-bit count (n uint32). */
int kwage_filterset_bit_counts(const kwage_filterset *fs, uint32_t *out);
/* Diagnostic: the first min(capacity, count) rows of filter i copied from the device; *count = the filter's set-bit
 * count.  Nothing on a search path calls it. */
int kwage_filterset_read_rows(const kwage_filterset *fs, uint32_t i, uint32_t *out, uint64_t capacity, uint64_t *count);

/* Filter search: cell (i, c) = the number of rows set in both filter i of the set and column c of the group; 0 for pad
 * columns and for an empty filter.
 *   - cells are uint32; cell (i, c) lies at scores[i*row_elems + c] for c in [0, kwage_group_column_span(g)); cells at
 *     or beyond the span in a row are not touched;
 *   - row_elems >= the span and row_elems % 4 == 0; scores_dev is 16-byte aligned.  Spans and the column bases of
 *     groups are multiples of 8 columns, so a caller places several groups side by side in one matrix by offsetting
 *     the pointer;
 *   - KWAGE_SEARCH_TIMING fills *search_kernel_ms (may be NULL) with the HIP-event duration of the score kernels;
 *     KWAGE_SEARCH_EARLY_EXIT is ignored: every column is counted to the end.
 * A set made from one group's columns searches any group of the same context with the same parameters.  Errors, all
 * found on the host before any kernel is launched: KWAGE_ERR_STATE before kwage_group_finalize; KWAGE_ERR_ARG when the
 * group's kmer_len, num_hash, log_2_filter_len or hash_func differ from the set's (filters built differently are not
 * comparable), for a sparse group, mixed contexts, a wrong row_elems, a misaligned or NULL pointer, or a set too large
 * for one launch.  The kernels are the dense score search's own, in their one-hash-function instantiations, over one row
 * per list entry.  Synchronous; runs on the context's first stream; device scratch comes from the context's pool.
 * The second form is the same search with the matrix copied to host memory. */
int kwage_search_filter_scores_device(kwage_group *g, kwage_filterset *fs, void *scores_dev, uint64_t row_elems,
                                      uint32_t flags, float *search_kernel_ms);
int kwage_search_filter_scores(kwage_group *g, kwage_filterset *fs, uint32_t *scores, uint64_t row_elems,
                               uint32_t flags, float *search_kernel_ms);
/* Which kernels the calling thread's last filter search launched: "score_tile_kernel<10,1>",
 * "count_kernel<7,1>+score_combine_kernel<14>"; "" if none.  Valid until the thread's next one. */
const char *kwage_search_filter_kernel(void);

/* The set-bit count of every column of a finalized, non-sparse group (the denominator of a Jaccard index): span uint32
 * cells, 0 on pad columns; the device form wants a 16-byte aligned pointer.  It is the filter search with one full
 * filter, whose row list 0, 1, .. 2^L - 1 is built on the device: KWAGE_ERR_ARG for L = 32 and for a sparse group,
 * KWAGE_ERR_STATE before finalize, KWAGE_ERR_DEVICE naming the row list when its 2^L x 4 bytes cannot be allocated. */
int kwage_group_column_bits(kwage_group *g, uint32_t *out);
int kwage_group_column_bits_device(kwage_group *g, void *out_dev);

/* The same search in two halves, for hosts that stream many batches: submit enqueues the whole device
 * pipeline and returns at once; collect waits for it and builds the result.  A context holds at most TWO
 * pending searches (each on its own HIP stream), so the k-mer stage, copy-back and host post-processing
 * of one batch overlap with the gather kernel of the other.  kwage_search == submit + collect. */
typedef struct kwage_pending kwage_pending;
int kwage_search_submit(kwage_group *g, kwage_batch *b, float threshold, uint32_t flags, kwage_pending **out);
int kwage_search_collect(kwage_pending *p, kwage_result **out);   /* consumes p, also on error */
/* 1 when collecting `p` would not wait any more (everything the search queued on the device has finished), 0 while it
 * would, < 0 on a device error.  For hosts that have other work to do meanwhile -- kwage_node feeds the context's slots
 * from inside its RCCL exchange with it.  Does not consume p. */
int kwage_search_poll(kwage_pending *p);

/* Device-side variant for multi-GPU hosts that exchange hit lists themselves (RCCL): hits are
 * left UNSORTED in the caller's device buffer of `capacity` records; *n_hits receives the total
 * found (which may exceed capacity: grow and call again).  num_query_kmer_dev may be NULL or a
 * device buffer of n_queries uint32. */
int kwage_search_device(kwage_group *g, kwage_batch *b, float threshold, uint32_t flags,
                        void *hits_dev, uint64_t capacity, uint64_t *n_hits,
                        void *num_query_kmer_dev);

/* The device-side search in two halves (see kwage_search_submit): the caller alternates between two hit
 * buffers so that the exchange of one step's hits overlaps with the next step's gather kernel.
 * count_dev may be NULL or a device uint64 that receives the total hit count in stream order behind
 * the search kernels -- an exchange buffer can then carry its own record count (header word followed
 * by the records) and go straight into an all-gather without any further device work. */
int kwage_search_device_submit(kwage_group *g, kwage_batch *b, float threshold, uint32_t flags,
                               void *hits_dev, uint64_t capacity, void *count_dev, kwage_pending **out);
/* search_kernel_ms (may be NULL): HIP-event duration of the gather kernel(s) when KWAGE_SEARCH_TIMING was set. */
int kwage_search_device_collect(kwage_pending *p, uint64_t *n_hits, void *num_query_kmer_dev, float *search_kernel_ms);

/* Append mode, for hosts whose result list spans several groups or shards -- the reference appends the matches of every
 * database file to one list per query (kwage.cpp:154-177): *count_dev (a device uint64, required) IS the list's hit
 * counter.  The search appends its records behind the ones already counted there instead of starting at record 0,
 * `column_base` is added to every reported column (each group / shard gets its own range of global column numbers),
 * and reset_count != 0 zeroes the counter in stream order before this search (the first search of a new list).
 * kwage_search_device_collect then reports the RUNNING total; records beyond `capacity` are counted, not stored
 * (grow the buffer and redo the list).  The searches of one context run in submission order. */
int kwage_search_device_append_submit(kwage_group *g, kwage_batch *b, float threshold, uint32_t flags,
                                      void *hits_dev, uint64_t capacity, void *count_dev, uint32_t column_base,
                                      int reset_count, kwage_pending **out);

/* K-mer stage alone (word.h:73-104 + kwage.cpp:362-366 + hash.cpp:176-234 on the device):
 * for query i writes its distinct canonical k-mers to kmers[kmer_offsets[i] ...] (unordered)
 * and their row indices to rows[(kmer_offsets[i]+j)*num_hash + h].  kmer_offsets must hold
 * n_queries+1 entries and is filled with the per-query capacity prefix (max(len-k+1,0));
 * num_query_kmer[i] receives the distinct count.  kmers / rows may be NULL. */
int kwage_hash_batch(kwage_ctx *ctx, const kwage_params *params, kwage_batch *b,
                     uint64_t *kmer_offsets, uint32_t *num_query_kmer,
                     uint64_t *kmers, uint32_t *rows);

/* Streaming-read microbenchmark over the group's bit matrix (achievable HBM peak on this box):
 * reads `bytes` (clamped to the matrix size) `iters` times; returns GB/s. */
int kwage_stream_read_gbps(kwage_group *g, uint64_t bytes, uint32_t iters, double *gbps);

/* ------------------------------------------------------------------------------------
 * Database construction (the format's only writer): replaces build_db() (build_db.cpp:24-456;
 * declared maestro.h:121) -- `.bloom` files in, one `.db` file out, byte-identical to the
 * reference's output; the bit transpose (build_db.cpp:259-304) runs on the device.
 * ---------------------------------------------------------------------------------- */
typedef struct {
	uint64_t bits_transposed;      /* 2^L * n                               */
	float transpose_kernel_ms;     /* sum over chunks, HIP events           */
	uint64_t db_bytes;             /* size of the file written              */
} kwage_build_stats;

int kwage_build_db(kwage_ctx *ctx, const char *out_path, const kwage_params *params,
                   const char *const *bloom_paths, uint32_t n, kwage_build_stats *stats);

/* ------------------------------------------------------------------------------------
 * Bloom filter construction from sequences -- the EXACT k-mer set (genomes / assemblies): every valid
 * canonical k-mer sets bit hash_h & (2^L - 1) for h < num_hash.  (The reference's make_bloom_filter()
 * always runs its counting-Bloom pass, which even at min_kmer_count == 1 may skip a k-mer whose counters
 * were raised by others; that behaviour, for any min_kmer_count, is kwage_bloom_counter_* below.)
 * Output: a `.bloom` file as binary_write<BloomFilter> writes it
 * (binary_io.cpp:182-208), ready for kwage_build_db.
 * ---------------------------------------------------------------------------------- */
typedef struct {
	const char *run_accession;                /* required: 3 letters + 1..10 digits (sra_accession.cpp:27-64) */
	const char *experiment_accession;         /* accessions and texts may be NULL or "" = absent */
	const char *sample_accession;
	const char *study_accession;
	const char *experiment_title;
	const char *experiment_design_description;
	const char *experiment_library_name;
	const char *experiment_library_strategy;
	const char *experiment_library_source;
	const char *experiment_library_selection;
	const char *experiment_instrument_model;
	const char *sample_taxa;
	const char *study_title;
	const char *study_abstract;
	const char *const *attribute_tags;        /* num_attributes entries each */
	const char *const *attribute_values;
	uint32_t num_attributes;
	uint64_t number_of_spots, number_of_bases;
	uint32_t day, month, year;                /* date_received; 0,0,0 = absent */
} kwage_sample_info;

/* optimal_bloom_param (bloom.cpp:10-68): smallest log_2_filter_len in [min,max], then the num_hash in
 * [1,5] with the lowest false-positive probability <= p for `num_kmer` distinct k-mers. */
int kwage_optimal_bloom_param(uint32_t kmer_len, uint64_t num_kmer, float p, uint32_t min_log_2_filter_len,
                              uint32_t max_log_2_filter_len, kwage_params *out);

/* Distinct canonical k-mers over ALL sequences of the batch (one shared set). */
int kwage_count_distinct_kmers(kwage_ctx *ctx, kwage_batch *b, uint32_t kmer_len, uint64_t *count);

/* Bits of the sample's Bloom filter (2^L / 8 bytes, LSB first) computed on the device. */
int kwage_bloom_bits_from_batch(kwage_ctx *ctx, const kwage_params *params, kwage_batch *b,
                                void *bits_out, uint64_t *distinct);

/* Sequences (concatenated + offsets, like kwage_batch_create) -> `.bloom` file. Long sequences are cut
 * into overlapping pieces internally so that every k-mer is seen once by some workgroup. */
int kwage_make_bloom(kwage_ctx *ctx, const kwage_params *params, const char *seqs, const uint64_t *offsets,
                     uint32_t n_seqs, const kwage_sample_info *info, const char *out_path,
                     uint64_t *num_distinct_kmers);

/* ------------------------------------------------------------------------------------
 * Bloom filter construction WITH a minimum k-mer count -- make_bloom_filter()'s counting pass
 * (make_bloom.cpp:76-504, count_words :506-621) with the reference's order-dependent semantics: two
 * 4-bit counting Bloom filters of 2^C elements with conservative update over the k-mer occurrences
 * of the read stream IN ORDER; the occurrence that lifts a k-mer's minimum counter to
 * min_kmer_count sets its five candidate bits in 2^M-bit vectors and counts as one k-mer; at the
 * end optimal_bloom_param(num_kmer) picks (log_2_filter_len, num_hash) and the first num_hash
 * vectors are OR-folded to that length (:336-354).  The device schedule commits occurrences that
 * share a counter in their original order, so counters, bits and num_kmer equal the sequential
 * loop's (kwage_amd/csrc/counter.hip).  Fragments are the sequences handed to _add, in call order
 * (the reference's front end -- NCBI SDK read iterators -- is replaced by whatever reads the caller
 * has, e.g. kwage_seqfile_*).  Note that even min_kmer_count == 1 differs from the exact k-mer set
 * of kwage_make_bloom: a new k-mer whose four counters were already raised by others is skipped.
 * PARITY UNPINNED against a running reference (make_bloom.cpp needs the NCBI SDK): checked against
 * the line-by-line restatement in oracle/.
 * ---------------------------------------------------------------------------------- */
typedef struct kwage_bloom_counter kwage_bloom_counter;

typedef struct {
	uint64_t num_valid_kmer;          /* m_progress.num_kmer                                      */
	uint64_t num_bp;                  /* m_progress.num_bp: bases of all fragments                */
	uint64_t positions;               /* k-mer start positions examined                           */
	uint64_t occurrences_committed;   /* occurrences that changed a counter                       */
	uint64_t chunks, rounds;          /* device chunks processed, commit rounds over all chunks   */
	uint32_t max_rounds;              /* longest commit chain in one chunk                        */
	uint32_t reserved;
	double add_ms;                    /* host wall time inside _add/_flush                        */
} kwage_bloom_counter_stats;

#define KWAGE_BLOOM_SUCCESS 0         /* STATUS_BLOOM_SUCCESS, maestro.h:25 */
#define KWAGE_BLOOM_INVALID 1         /* STATUS_BLOOM_INVALID, maestro.h:27: bound not satisfiable / no k-mers */

/* make_bloom.cpp:105-130: log2 length of the counting filters from the number of bases (0 = unknown -> 32). */
uint32_t kwage_counting_filter_log2(uint64_t num_bp);
/* bloom.cpp:72-121 approximate_max_kmers */
uint64_t kwage_approximate_max_kmers(float false_positive_probability, uint32_t min_log_2_filter_len,
                                     uint32_t max_log_2_filter_len);

int kwage_bloom_counter_create(kwage_ctx *ctx, uint32_t kmer_len, int32_t hash_func, uint32_t min_kmer_count,
                               uint32_t log_2_counting_filter_len, uint32_t max_log_2_filter_len,
                               kwage_bloom_counter **out);
void kwage_bloom_counter_destroy(kwage_bloom_counter *bc);
/* Next sample in the same object (device allocations kept; a 2^32-element object costs ~20 GB to create):
 * counters, candidate bits and totals are zeroed; the counting filters may be smaller than at creation. */
int kwage_bloom_counter_reset(kwage_bloom_counter *bc, uint32_t min_kmer_count, uint32_t log_2_counting_filter_len);
/* Append fragments (concatenated + offsets, like kwage_batch_create) to the read stream. */
int kwage_bloom_counter_add(kwage_bloom_counter *bc, const char *seqs, const uint64_t *offsets, uint32_t n_seqs);
/* Process what is staged on the host so far (add() works in 16 M-position chunks). */
int kwage_bloom_counter_flush(kwage_bloom_counter *bc);
int kwage_bloom_counter_get_stats(kwage_bloom_counter *bc, kwage_bloom_counter_stats *out);
/* Inspection (tests): CountingBloom elements [first, first+n) as bytes (low nibble `first`, high nibble
 * `second`, make_bloom.cpp:59-66) and bytes of candidate bit vector `hash` (LSB first). */
int kwage_bloom_counter_read_counts(kwage_bloom_counter *bc, uint64_t first, uint64_t n, void *out);
int kwage_bloom_counter_read_valid_bits(kwage_bloom_counter *bc, uint32_t hash, uint64_t first_byte, uint64_t nbytes, void *out);
/* make_bloom.cpp:210-216,309-450: *status = KWAGE_BLOOM_INVALID (nothing written) if num_kmer exceeds
 * approximate_max_kmers or no parameters satisfy the bound; else fold, CRC and write the `.bloom` file
 * (out_path may be NULL: parameters only).  `chosen` may be NULL. */
int kwage_bloom_counter_finish(kwage_bloom_counter *bc, float false_positive_probability, uint32_t min_log_2_filter_len,
                               const kwage_sample_info *info, const char *out_path, kwage_params *chosen, int *status);

/* Column-wise re-pack: the columns of several same-parameter `.db` files (raw or compressed) become
 * ONE raw `.db` file with contiguous columns, in file order then column order -- the bit-level work of
 * the reference's merge_db.cpp:268-820 (get_bit/set_bit per bit there; shift-and-OR on the device
 * here), without its file naming / size policy.  The reference `kwage` reads the result. */
int kwage_repack_db(kwage_ctx *ctx, const char *out_path, const char *const *in_paths, uint32_t n);

/* Save, no counterpart in the reference: `n` columns of the group's resident matrix, in the order listed, written as ONE
 * raw `.db` file (compression 0) -- file blocks, live inserts at bit granularity, what is left around retired columns.
 * The columns are gathered and packed densely on the device; the file is byte for byte what kwage_build_db writes from
 * the same Bloom filters and metadata in the same order, so a save followed by a load also defragments what
 * kwage_group_retire_columns leaves (kwage_group_compact does that in place, without the file).
 *   - cols[i].column is a global column of the group and becomes column i of the file.  Its FilterInfo record is copied
 *     verbatim from column source_column of the `.db` / `.dbz` file source_db (as kwage_repack_db copies records; each
 *     distinct file is opened once), or, when source_db is NULL, serialized from *info as kwage_make_bloom serializes it;
 *   - staging_bytes: the size of one chunk of output rows in pinned host memory (two such blocks, used alternately: a
 *     chunk's CRC32 and file write run on a host thread beside the next chunk's kernel and copy); 0 means 64 MiB, and any
 *     value works, down to one row per chunk;
 *   - the file is written under a temporary name beside out_path and renamed at the end: a failure on the device or on
 *     disk leaves no partial file and an existing out_path as it was; out_path may name one of the source_db files;
 *   - the group, its valid mask and its span are not changed; before and after kwage_group_finalize;
 *   - stats may be NULL.
 * Errors, all found before out_path is touched: KWAGE_ERR_ARG for a NULL argument, n == 0, a sparse group (its matrix
 * holds only some rows), a column at or beyond the span, a pad or retired column, a column listed twice, an entry with
 * neither source_db nor info, a source_column beyond its file; KWAGE_ERR_STATE while a search is pending on the context;
 * KWAGE_ERR_IO / KWAGE_ERR_FORMAT for an unreadable or damaged source of metadata.
 * Synchronous; runs on the context's first stream. */
typedef struct {
	uint64_t column;                 /* global column of the group                                              */
	const char *source_db;           /* copy this column's FilterInfo record verbatim from column source_column */
	uint32_t source_column;          /*   of this .db / .dbz file ...                                           */
	const kwage_sample_info *info;   /* ... or, when source_db is NULL, serialize this (as kwage_make_bloom does) */
} kwage_save_column;

typedef struct {
	uint64_t db_bytes;               /* size of the file written            */
	uint64_t runs;                   /* runs the column list folded into    */
	uint32_t chunks;                 /* staged chunks of rows               */
	float extract_kernel_ms;         /* sum over chunks, HIP events         */
} kwage_save_stats;

int kwage_group_save_db(kwage_group *g, const char *out_path, const kwage_save_column *cols, uint32_t n,
                        uint64_t staging_bytes, kwage_save_stats *stats);

/* Export, no counterpart in the reference (which has dump_bloom / dump_db to look at such objects): `n` columns of the
 * group's resident matrix handed back as what they were made from -- whole Bloom filters, filter-major, 2^L bits each,
 * LSB first: the payload of a `.bloom` file, exactly the layout kwage_group_insert_filters and kwage_filterset_from_bits
 * read -- transposed on the device.  The inverse of the live insert: a sample of a resident database can be moved to
 * another group, re-inserted after a rebuild, or written as the `.bloom` file it was built from.
 *   - columns[i] is a global column of the group and becomes filter i of the output; the list may be in any order and may
 *     name a column more than once (it is then written more than once);
 *   - filter i lies at bits + i*filter_stride_bytes (the stride is ignored when n < 2) and is max(1, 2^L / 8) bytes; for
 *     L < 3 it is one byte whose bits at and above 2^L are written as zero.  Exactly the filters' bytes are written:
 *     nothing between or behind them is touched, and nothing has to be cleared beforehand.  One thread owns an (output
 *     filter, 32 rows): no atomics, no read of the output;
 *   - the group, its matrix, valid mask and span are not changed; before and after kwage_group_finalize;
 *   - flags: KWAGE_SEARCH_TIMING fills *export_kernel_ms (may be NULL) with the HIP-event duration of the export kernels
 *     summed over chunks; other bits are ignored.
 * The host form stages chunks of rows -- rows [r0, r0 + nr), nr a multiple of 8 -- through the context's load buffer;
 * a chunk's n x nr/8 bytes leave the device with one strided copy, to bits + i*filter_stride_bytes + r0/8.  staging_bytes
 * bounds a chunk: 0 means 64 MiB, and any value works, down to one byte of every filter per chunk.  The device form
 * writes device memory in place; pointer and stride must be multiples of 4.  The file form writes n `.bloom` files (magic,
 * the group's BloomParam, CRC32 of the bits, FilterInfo record, bits), filter i to out_paths[i]; the record comes from
 * cols[i] exactly as kwage_group_save_db takes it.  Every file is written under a temporary name beside its destination
 * and all n are renamed only once all are complete: a failure on the device or on disk leaves no partial file, no
 * temporary file, and an existing destination as it was.
 * Errors, all found before a byte of the caller's memory or of any file is written: KWAGE_ERR_ARG for a NULL argument,
 * n == 0, a sparse group, a column at or beyond the span, a pad or retired column, a filter_stride_bytes smaller than a
 * filter with n > 1, a device pointer or stride that is not a multiple of 4, an entry with neither source_db nor info, a
 * source_column beyond its file, a NULL path; KWAGE_ERR_STATE while a search is pending on the context; KWAGE_ERR_IO /
 * KWAGE_ERR_FORMAT for an unreadable or damaged source of metadata.  Synchronous; runs on the context's first stream. */
int kwage_group_export_filters(kwage_group *g, const uint64_t *columns, uint32_t n, void *bits,
                               uint64_t filter_stride_bytes, uint64_t staging_bytes, uint32_t flags, float *export_kernel_ms);
int kwage_group_export_filters_device(kwage_group *g, const uint64_t *columns, uint32_t n, void *bits_dev,
                                      uint64_t filter_stride_bytes, uint32_t flags, float *export_kernel_ms);
int kwage_group_export_bloom_files(kwage_group *g, const kwage_save_column *cols, const char *const *out_paths, uint32_t n,
                                   uint64_t staging_bytes, uint32_t flags, float *export_kernel_ms);

/* ------------------------------------------------------------------------------------
 * Host-side helpers that mirror the reference's host code for this path (no device needed).
 * ---------------------------------------------------------------------------------- */

/* DBFileHeader, kwage.h:30-72, as serialized by binary_io.cpp:243-265 (44 bytes, LE). */
typedef struct {
	uint32_t magic, version, crc32, kmer_len, num_hash, log_2_filter_len, num_filter;
	int32_t  hash_func;
	uint32_t compression;
	uint64_t info_start;
} kwage_db_header;

int kwage_db_read_header(const char *path, kwage_db_header *out);

/* The listed slices of one .db file (host only; raw or compressed), n * ceil(num_filter / 8) bytes in list order:
 * what the reference's seekg + read per addressed slice fetches (kwage.cpp:414-416), and what the sparse groups
 * (kwage_group_create_sparse) are loaded through -- several threads for long lists. */
int kwage_db_read_slices(const char *path, const uint32_t *rows, uint64_t n, unsigned char *out);

/* Compressed container (host only).  The reference ships a slice CODEC (slice_z.h: raw deflate,
 * windowBits -9, level 9, memLevel 9, default strategy, "store raw unless smaller") but no file
 * layout, and its kwage ignores header.compression.  This repo defines the layout:
 * header.compression = 2, u64 offset[2^L+1], per-slice payloads, then the usual metadata.
 * kwage_group_add_db_file reads both layouts (slices are inflated once, on the host, at load).
 * Parity with the reference is UNPINNED for this container (it has none); it is validated by
 * round trip: decompress(compress(x)) == x byte for byte, and identical search results. */
int kwage_db_compress(const char *in_path, const char *out_path, uint32_t threads);
int kwage_db_decompress(const char *in_path, const char *out_path);

/* Database metadata reader: info_loc[] + FilterInfo records (kwage.cpp:505-515,
 * binary_io.cpp:154-176), loaded once per file instead of two seeks per hit. */
typedef struct kwage_dbinfo kwage_dbinfo;
int kwage_dbinfo_open(const char *path, kwage_dbinfo **out);
void kwage_dbinfo_close(kwage_dbinfo *d);
uint32_t kwage_dbinfo_num_filter(const kwage_dbinfo *d);
/* FilterInfo::csv_string() (bloom.cpp:124-127): the run accession. */
int kwage_dbinfo_csv_string(const kwage_dbinfo *d, uint32_t column, char *buf, size_t buflen);
/* FilterInfo::json_string(prefix) (bloom.cpp:129-326). Returns needed length (excluding NUL). */
int64_t kwage_dbinfo_json_string(const kwage_dbinfo *d, uint32_t column, const char *prefix,
                                 char *buf, size_t buflen);

/* sra_accession.cpp:27-96 */
int kwage_str_to_accession(const char *s, uint64_t *out);
int kwage_accession_to_str(uint64_t acc, char *buf, size_t buflen);

/* SequenceIterator (parse_sequence.cpp:13-262): FASTA / FASTQ, gz transparent. */
typedef struct kwage_seqfile kwage_seqfile;
int kwage_seqfile_open(const char *path, kwage_seqfile **out);
/* Returns 1 and sets the views (valid until the next call) or 0 at end of file, <0 on error. */
int kwage_seqfile_next(kwage_seqfile *f, const char **defline, const char **seq, uint64_t *seq_len);
void kwage_seqfile_close(kwage_seqfile *f);

/* (unsigned)(float threshold * n), kwage.cpp:388 */
uint32_t kwage_query_threshold(float threshold, uint32_t num_query_kmer);

#ifdef __cplusplus
}
#endif

#endif /* KWAGE_AMD_H */
