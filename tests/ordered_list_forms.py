"""Every gather-kernel form that reserves hit slots, driven to a long list whose order is known in closed form: a matrix
of identical rows, so a query with a k-mer reports exactly the columns that are all ones, ascending.  The table of knobs
and kernel names is shared by test_gpu_parity.py (every column but each seventh) and test_gpu_hit_order.py (irregular
columns: run lengths differ from run to run and many runs are empty)."""
import numpy as np

L, K = 6, 31
LIVE_SHARE = 1 - (1 / 9 + 1 / 13 - 1 / 117)      # of the queries made below, those with a k-mer


def rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


NARROW_MIN_QUERIES = 64      # engine.hip: the several-queries-per-wave kernels take batches of 64 queries or more


def queries_for(n_ones, at_least=24, margin=1.15):
    """Queries that give more than 8192 records when each live one reports n_ones columns."""
    return max(at_least, int((8192 // n_ones + 2) / LIVE_SHARE * margin) + 6)


def drive_every_kernel_form(ka, ctx, n_cols, ones, n_queries, seed):
    """`ones`: bool [n_cols], the columns that are all ones (the others are all zero).  Returns the kernel names checked."""
    nbytes = (n_cols + 7) // 8
    bits = np.zeros(nbytes * 8, dtype=np.uint8)
    bits[:n_cols] = ones
    row = np.packbits(bits.reshape(nbytes, 8), axis=1, bitorder="little").reshape(-1)
    image = np.ascontiguousarray(np.tile(row, (1 << L, 1)))
    one_cols = np.flatnonzero(ones).astype(np.uint32)
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(n_queries):
        # (at most 120 k-mers: no automatic row-list segments; at least 3: a threshold that truncates to 0 would report the zero columns too)
        n = int(rng.choice([33, 35, 40, 64, 100, 150]))
        seqs.append("ACGT" if i % 9 == 4 else ("N" * n if i % 13 == 5 else rand_seq(rng, n)))
    g = ka.Group(ctx, K, 2, L, n_cols)
    g.add_columns(image, n_cols)
    g.finalize()
    b = ka.Batch(ctx, seqs)
    seen = []

    def check(r, want_kernel):
        assert r.search_kernel.startswith(want_kernel), (r.search_kernel, want_kernel)
        seen.append(want_kernel)
        nk = r.num_query_kmer
        live = np.flatnonzero(nk > 0).astype(np.uint32)
        # (above 8192 records is a condition: shorter lists are sorted by the host, and nothing of the run table is tested)
        assert len(live) >= n_queries // 2 and len(r.hits) == len(live) * len(one_cols) > 8192
        assert np.array_equal(r.hits["query"], np.repeat(live, len(one_cols))), want_kernel
        assert np.array_equal(r.hits["column"], np.tile(one_cols, len(live))), want_kernel
        assert np.array_equal(r.hits["num_match"], np.repeat(nk[live], len(one_cols))), want_kernel

    units = (nbytes + 127) // 128 * 8
    off = dict(walk=0, count_walk=0, narrow=0, force_segs=0, walk_bands=0)
    if units <= 32:
        with ctx.tuning(**dict(off, narrow=1)):
            check(g.search(b, 1.0), "and_narrow_kernel<")
            if units > 8:
                check(g.search(b, 0.5), "count_narrow_kernel<")
    for vec in (1, 2, 4):
        with ctx.tuning(**dict(off, and_vec=vec)):
            check(g.search(b, 1.0), "and_kernel<%d," % vec)
    with ctx.tuning(**dict(off, force_segs=3)):
        check(g.search(b, 1.0), "and_kernel<")
        assert g.search(b, 1.0).search_kernel.endswith("+segments")
        check(g.search(b, 0.5), "count_kernel<")
    with ctx.tuning(**off):
        check(g.search(b, 0.5), "count_kernel<")
    if units >= 64:
        # early exit, every tile handed over to the refine launch after its first eight rows: one reservation per cluster
        # (= per query and KiB-step), by the emit launch; and with lists of three places: most tiles walk on by themselves
        for knobs in (dict(refine_max_groups=16, refine_min_rows=1, refine_seg_rows=8), dict(refine_max_groups=16, refine_min_rows=1, refine_list_cap=3)):
            with ctx.tuning(**dict(off, count_screen_min_tiles=1, **knobs)):
                check(g.search(b, 1.0, ka.SEARCH_EARLY_EXIT), "and_screen_kernel<")
                check(g.search(b, 0.5, ka.SEARCH_EARLY_EXIT), "count_screen_kernel<")
    for waves in (0, 37):
        with ctx.tuning(**dict(off, count_walk=1, count_walk_min_rows=1, count_walk_waves=waves)):
            check(g.search(b, 0.5), "count_walk_kernel<")
        if units >= 2 * 64:
            with ctx.tuning(**dict(off, walk=4, walk_min_rows=1, walk_max_kib=64, walk_waves=waves)):
                check(g.search(b, 1.0), "and_walk_kernel<")
            if units <= 16 * 64:
                with ctx.tuning(**dict(off, walk=4, walk_min_rows=1, walk_waves=waves, walk_bands=3, walk_bands_min_gib=0)):
                    check(g.search(b, 1.0), "and_band_walk_kernel<")
    b.close()
    g.close()
    return seen
