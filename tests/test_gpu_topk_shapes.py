"""kwage_search_topk at every shape the library can launch, against the exact reference of topk_reference.py (the CPU
oracle's counts, the oracle's floor, the contract's selection): every counter width (7 / 10 / 14 / 20 / 32 planes) and
hash count in the tile and the segmented form, batches cut into several slices (candidate-bound and slab-bound), small
and tile-boundary groups, sparse groups, and the k-mer layout a top-k search shares with kwage_search.

Every case asserts the kernel instantiation it meant to reach (res.search_kernel), so a change of dispatch cannot turn
it into a duplicate of another.  KWAGE_TOPK_FULL_GRID=1 runs the whole k x t grid at every (width, hash count)."""
import os
import re

import numpy as np
import pytest

import topk_reference as ref
from topk_reference import assert_hits_equal, column_counts, expected_hits, pack_columns, rand_bits, rand_seq

pytestmark = pytest.mark.gpu

FULL_GRID = os.environ.get("KWAGE_TOPK_FULL_GRID", "0") == "1"
KS = (1, 2, 63, 64, 65, 256, 257, 1024)


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def ctx(ka):
    c = ka.Context(0)
    yield c
    c.close()


def planes(max_count):
    """The narrowest instantiated counter width holding counts up to max_count."""
    return next(p for p in (7, 10, 14, 20, 32) if max_count < (1 << p))


def tile_name(p, nh):
    return "topk_tile_kernel<%d,%d>" % (p, nh)


def assert_combine(name, p, nh):
    m = re.match(r"count_kernel<(\d+),(\d+)>\+topk_combine_kernel<(\d+)>", name)
    assert m and int(m.group(2)) == nh and int(m.group(3)) == p and int(m.group(1)) <= p, (name, p, nh)


def set_col(bits, rows, col, value=True):
    bits[rows, col] = value


def add_files(ka, ctx, kmer, nh, L, images):
    """images: [(packed image, nf, column_map)] -> finalized group, reference files, column span."""
    g = ka.Group(ctx, kmer, nh, L, sum(((nf + 127) // 128) * 128 for _, nf, _ in images))
    files = []
    for img, nf, cmap in images:
        first = g.add_columns(img if cmap is None else img[1], nf)
        files.append((first, img if cmap is None else img[0], nf, cmap))
    g.finalize()
    return g, files, g.column_span


def copies(rng, base_bits, nf, shift):
    """A file of nf columns, column j a copy of base column (j * 7 + shift) % B: (packed base, packed file), map."""
    B = base_bits.shape[1]
    cmap = ((np.arange(nf, dtype=np.int64) * 7 + shift) % B).astype(np.int64)
    return (pack_columns(base_bits, rng), pack_columns(base_bits[:, cmap], rng)), nf, cmap


def reference(oracle, files, span, kmer, nh, L, queries):
    out = []
    for q in queries:
        kmers = oracle.unique_kmers(q, kmer)
        out.append((len(kmers), column_counts(oracle, files, span, kmer, nh, L, kmers)))
    return out


def check(ka, oracle, g, b, per_query, k, t, what, kernel=None):
    res = ka.search_topk(g, b, k, t)
    exp, floors = expected_hits(oracle, per_query, t, k)
    assert np.array_equal(res.num_query_kmer, [n for n, _ in per_query]), what
    assert np.array_equal(res.query_threshold, floors), what
    assert_hits_equal(res.hits, exp, "%s k=%d t=%g %s" % (what, k, t, res.search_kernel))
    if kernel is not None:
        kernel(res.search_kernel)
    return res


# ---- 1. counter width x hash count ----------------------------------------------------------------------------------
WIDTHS = (127, 128, 1023, 1024, 16383, 16384)
FULL_POINTS = {(127, 1), (1024, 2), (16383, 3), (128, 4), (16384, 5)}


@pytest.mark.parametrize("nh", [1, 2, 3, 4, 5])
def test_every_counter_width_and_hash_count(ka, ctx, oracle, nh):
    rng = np.random.default_rng(1000 + nh)
    kmer, L = 31, 14
    genome = rand_seq(rng, max(WIDTHS) + kmer - 1)
    full_rows = oracle.row_indices(oracle.unique_kmers(genome, kmer), kmer, nh, L).reshape(-1)
    half_rows = oracle.row_indices(oracle.unique_kmers(genome[:8000 + kmer - 1], kmer), kmer, nh, L).reshape(-1)
    density = (0.3, 0.55, 0.7, 0.78, 0.82)[nh - 1]
    images = []
    for nf, full, half, dups in ((3001, (5, 3000), (7, 2999), ((17, 18), (17, 2500))),
                                 (8667, (5119, 5120, 8000), (5121, 8666), ((100, 5119 + 40), (4000, 5200)))):
        bits = rand_bits(rng, (1 << L, nf), density)
        for c in full:                                   # every row of the longest query: some score reaches n
            set_col(bits, full_rows, c)
        for c in half:                                   # equal partial columns, in two files and three tiles
            set_col(bits, half_rows, c)
        for a, c in dups:
            bits[:, c] = bits[:, a]
        images.append((pack_columns(bits, rng), nf, None))
    g, files, span = add_files(ka, ctx, kmer, nh, L, images)
    assert span > 8192 + 128                             # two tiles of 8192 columns at least
    try:
        for P in WIDTHS:
            longest = genome[:P + kmer - 1]
            queries = [longest, genome[17:17 + min(100, P)], rand_seq(rng, 90), "ACGTACGT", genome[300:300 + P // 2 + kmer - 1]]
            per_query = reference(oracle, files, span, kmer, nh, L, queries)
            assert per_query[0][0] == P                          # random sequence: every position a distinct k-mer
            assert per_query[0][1].max() == P                    # planted: the top plane bit is set
            p = planes(P)
            b = ka.Batch(ctx, queries)
            grid = [(k, t) for k in KS for t in (0.0, 0.5, 1.0)] if (FULL_GRID or (P, nh) in FULL_POINTS) else \
                [(1, 0.5), (65, 0.5), (1024, 0.5)]
            try:
                for segs in (1, 0, 3):
                    def kernel(name):
                        if segs == 1 or (segs == 0 and "topk_tile_kernel" in name):
                            assert name.startswith(tile_name(p, nh)), (name, p, nh)
                        else:
                            assert_combine(name, p, nh)
                    with ctx.tuning(force_segs=segs):
                        for k, t in grid:
                            check(ka, oracle, g, b, per_query, k, t, "P=%d nh=%d segs=%d" % (P, nh, segs), kernel)
            finally:
                b.close()
    finally:
        g.close()


# ---- 2. queries above 2^20 positions ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_batch(ka, ctx, oracle):
    rng = np.random.default_rng(1 << 20)
    genome = rand_seq(rng, 1_150_000)
    queries = [rand_seq(rng, 400), genome, "ACG", genome[1000:1500]]
    b = ka.Batch(ctx, queries)
    yield queries, b, [oracle.unique_kmers(q, 31) for q in queries]
    b.close()


@pytest.mark.parametrize("nh", [1, 5])
def test_queries_above_2_pow_20_positions(ka, ctx, oracle, long_batch, nh):
    queries, b, kmers = long_batch
    rng = np.random.default_rng(77 + nh)
    kmer, L, B = 31, 10, 120
    base = rand_bits(rng, (1 << L, B), (0.5 if nh == 1 else 0.85))
    base[:, [4, 60]] = True                              # every row: the score n > 2^20 needs the 32-bit counters
    base[: (1 << L) // 2, 9] = True                      # a partial column, copied across both tiles
    # the second file: copies of the base across 8192 columns (ties at every score, in both tiles)
    g, files, span = add_files(ka, ctx, kmer, nh, L, [(pack_columns(base, rng), B, None), copies(rng, base, 8300, 11)])
    try:
        per_query = []
        for km in kmers:
            per_query.append((len(km), column_counts(oracle, files, span, kmer, nh, L, km)))
        assert per_query[1][0] > 1 << 20 and per_query[1][1].max() == per_query[1][0]
        for segs in (0, 1):
            with ctx.tuning(force_segs=segs):
                for k in (1, 64, 1024):
                    for t in (0.0, 0.9):
                        def kernel(name):
                            if segs == 0:       # the default: segments + the combine form with 64 KiB of LDS
                                assert_combine(name, 32, nh)
                            else:
                                assert name.startswith(tile_name(32, nh)), name
                        check(ka, oracle, g, b, per_query, k, t, "nh=%d segs=%d" % (nh, segs), kernel)
    finally:
        g.close()


# ---- 3 / 4. batches cut into several slices -----------------------------------------------------------------------------
def sample_of_slices(n, slice_q, every):
    s = set(range(0, n, every)) | {n - 1}
    for q0 in range(0, n, slice_q):
        s |= {q0, min(n, q0 + slice_q) - 1}
    return sorted(s)


def check_sliced(ka, oracle, g, b, files, span, kmer, nh, L, queries, k, sample, what, kernel, knobs=None):
    """Every query against the device threshold search at t = 0.5 cut at k (itself pinned to the oracle by the parity
    suite), the sampled queries against the reference at t = 0 and 0.5; records carry the global query index."""
    thr = g.search(b, 0.5)                                       # (the library's own choice of threshold kernel)
    per_query = {q: reference(oracle, files, span, kmer, nh, L, [queries[q]])[0] for q in sample}
    launches = []
    for t in (0.5, 0.0):
        with ctx_tuning(g, knobs):
            res = ka.search_topk(g, b, k, t)
        kernel(res.search_kernel)
        launches.append(res.search_kernel_launches)
        assert res.search_kernel_launches >= 3, (what, res.search_kernel_launches)
        assert np.array_equal(res.num_query_kmer, thr.num_query_kmer), what
        if t == 0.5:
            assert_hits_equal(res.hits, ref.cut_threshold_hits(thr.hits, k), what + " vs threshold search")
        for q in sample:
            got = res.hits[res.hits["query"] == q]
            exp, floors = expected_hits(oracle, [per_query[q]], t, k)
            exp["query"] = q
            assert res.query_threshold[q] == floors[0] and res.num_query_kmer[q] == per_query[q][0], (what, q)
            assert_hits_equal(got, exp, "%s t=%g q=%d" % (what, t, q))
    return res, launches


def ctx_tuning(g, knobs):
    return g.ctx.tuning(**(knobs or {}))


def test_sliced_batch_candidate_bound(ka, ctx, oracle):
    """~300 000 columns x k = 1024: the candidate buffer holds ~880 queries, 2000 reads make three slices."""
    rng = np.random.default_rng(31)
    kmer, nh, L, B = 31, 1, 10, 3001
    base = rand_bits(rng, (1 << L, B), 0.4)
    genome = rand_seq(rng, 60000)
    full = oracle.row_indices(oracle.unique_kmers(genome, kmer), kmer, nh, L).reshape(-1)
    base[full, 3] = True                                          # every read of the genome scores n here ...
    base[full, 1000] = True
    base[:, 2000] = base[:, 5]                                    # ... and equal columns, copied into every tile
    images = [copies(rng, base, nf, shift) for nf, shift in ((74999, 0), (75001, 1), (80000, 2), (70003, 1500))]
    g, files, span = add_files(ka, ctx, kmer, nh, L, images)
    chunks = -(-g.row_stride // 16 // 64)
    slice_q = (256 << 20) // (chunks * 1024 * 8)
    n = 2000
    assert 3 * slice_q > n > 2 * slice_q, slice_q                 # three slices, the last partial
    starts = rng.integers(0, len(genome) - 200, size=n)
    lens = rng.integers(120, 200, size=n)
    queries = [genome[s:s + ln] if i % 5 else rand_seq(rng, int(ln)) for i, (s, ln) in enumerate(zip(starts, lens))]
    no_kmers = (slice_q + 7, n - 2)                                # shorter than k, in the second and the last slice
    for q in no_kmers:
        queries[q] = "ACGTACGTAC"
    b = ka.Batch(ctx, queries)
    try:
        res, _ = check_sliced(ka, oracle, g, b, files, span, kmer, nh, L, queries, 1024,
                              sample_of_slices(n, slice_q, 97) + list(no_kmers), "candidate-bound",
                              lambda name: name.startswith(tile_name(10, 1)) or pytest.fail(name))
        for q in no_kmers:
            assert res.num_query_kmer[q] == 0 and not (res.hits["query"] == q).any()
    finally:
        b.close()
        g.close()


def test_sliced_batch_slab_bound(ka, ctx, oracle):
    """Long queries over ~350 000 columns with 1000+ forced segments: the slab of partial counters holds three
    queries, eight make three slices; shorter queries in later slices use fewer segments than the launch has."""
    rng = np.random.default_rng(41)
    kmer, nh, L, B = 31, 1, 8, 5003
    base = rand_bits(rng, (1 << L, B), 0.5)
    base[:, 77] = True                                            # every row: the score n, copied into every tile
    images = [copies(rng, base, nf, shift) for nf, shift in ((100003, 0), (90000, 3), (85007, 9), (75000, 2500))]
    g, files, span = add_files(ka, ctx, kmer, nh, L, images)
    genome = rand_seq(rng, 72000)
    P = (70000, 64000, 52000, 50000, 0, 41000, 30000, 0)
    queries = [genome[i * 100:i * 100 + p + kmer - 1] if p else "ACGT" for i, p in enumerate(P)]
    segs = 1024
    seg_kmers = -(-max(P) // segs)
    slab_q = (1 << 30) // (-(-max(P) // seg_kmers) * planes(seg_kmers) * g.row_stride)
    assert slab_q == 3, slab_q                                     # slices (3, 3, 2): n = 0 in the second and the last
    b = ka.Batch(ctx, queries)
    try:
        _, launches = check_sliced(ka, oracle, g, b, files, span, kmer, nh, L, queries, 1024, list(range(len(P))),
                                   "slab-bound", lambda name: assert_combine(name, 20, 1), dict(force_segs=segs))
        assert launches == [3, 3], launches
        check_sliced(ka, oracle, g, b, files, span, kmer, nh, L, queries, 65, [0, 2, 3, 5, 6, 7], "slab-bound k=65",
                     lambda name: assert_combine(name, 20, 1), dict(force_segs=segs))
    finally:
        b.close()
        g.close()


# ---- 5. small and tile-boundary groups ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 7, 127, 128, 129, 8191, 8192, 8193])
def test_small_and_boundary_width_groups(ka, ctx, oracle, nf):
    rng = np.random.default_rng(nf)
    kmer, nh, L = 31, 2, 9
    bits = rand_bits(rng, (1 << L, nf), 0.75)
    if nf > 3:
        bits[:, nf - 1] = bits[:, 0]
    g, files, span = add_files(ka, ctx, kmer, nh, L, [(pack_columns(bits, rng), nf, None)])
    genome = rand_seq(rng, 400)
    queries = [genome, genome[100:250], rand_seq(rng, 60), "ACG"]
    per_query = reference(oracle, files, span, kmer, nh, L, queries)
    b = ka.Batch(ctx, queries)
    try:
        for segs in (1, 3):
            with ctx.tuning(force_segs=segs):
                for k in sorted({min(max(1, x), 1024) for x in (1, nf - 1, nf, nf + 1, 1024)}):
                    for t in (0.0, 0.5):
                        res = check(ka, oracle, g, b, per_query, k, t, "nf=%d segs=%d" % (nf, segs),
                                    (lambda name: name.startswith(tile_name(planes(370), 2)) or pytest.fail(name)) if segs == 1
                                    else (lambda name: assert_combine(name, planes(370), 2)))
                        assert (res.hits["column"] < nf).all()             # never a pad column
                        if t == 0.0 and k >= nf:                            # every real column of every query with k-mers
                            for q in range(3):
                                assert (res.hits["query"] == q).sum() == nf
    finally:
        b.close()
        g.close()


# ---- 6. sparse groups ------------------------------------------------------------------------------------------------
def test_sparse_group_top_k(ka, ctx, oracle, tmp_path):
    import torch
    from kwage_amd import native
    rng = np.random.default_rng(99)
    kmer, nh, L = 31, 3, 13
    genome = rand_seq(rng, 2500)
    grow = oracle.row_indices(oracle.unique_kmers(genome, kmer), kmer, nh, L).reshape(-1)
    paths, images = [], []
    for f, nf in enumerate((2048, 100, 30000, 2048)):
        bits = rand_bits(rng, (1 << L, nf), 0.8)
        for c in (7 + f, nf - 1):
            bits[grow, c] = True
        img = np.packbits(np.pad(bits, ((0, 0), (0, (-nf) % 8))), axis=1, bitorder="little")
        p = str(tmp_path / ("s%d.db" % f))
        infos = [oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%07d" % (f * 100000 + j))) for j in range(nf)]
        oracle.write_db(p, kmer, nh, L, img, nf, infos)
        if f == 1:                                                  # one of them in the compressed container
            z = str(tmp_path / "s1.dbz")
            native.check(native.lib().kwage_db_compress(p.encode(), z.encode(), 2))
            p = z
        paths.append(p)
        images.append((img, nf))
    cap = sum(((nf + 127) // 128) * 128 for _, nf in images)
    queries = [genome[100:600], rand_seq(rng, 300), genome[1000:1200].lower(), "ACGT", rand_seq(rng, 150), genome[:2000]]
    b = ka.Batch(ctx, queries)
    _, rows = ka.hash_batch(ctx, kmer, nh, L, b)
    need = np.unique(np.concatenate([r.reshape(-1) for r in rows]))
    full = ka.Group(ctx, kmer, nh, L, cap)
    firsts = full.add_db_files(paths)
    full.finalize()
    sp = ka.Group.sparse(ctx, kmer, nh, L, cap, need)
    assert sp.add_db_files(paths) == firsts
    sp.finalize()
    files = [(first, np.ascontiguousarray(img), nf, None) for (first, _), (img, nf) in zip(firsts, images)]
    per_query = reference(oracle, files, full.column_span, kmer, nh, L, queries)
    hits = torch.zeros((len(queries) * 1024, 3), dtype=torch.int32, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    other = ka.Batch(ctx, [rand_seq(rng, 400)])
    try:
        def both(k, t, what):
            a = check(ka, oracle, full, b, per_query, k, t, what)
            c = ka.search_topk(sp, b, k, t)
            assert c.search_kernel == a.search_kernel, (c.search_kernel, a.search_kernel)
            assert np.array_equal(c.hits, a.hits) and np.array_equal(c.num_query_kmer, a.num_query_kmer), what
            assert np.array_equal(c.query_threshold, a.query_threshold), what
            total = ka.search_topk_device_append(sp, b, k, hits, count, column_base=1000, threshold=t)
            assert total == c.hits.size == int(count.item())
            got = hits[:total].cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:, 0], c.hits["query"]) and np.array_equal(got[:, 1], c.hits["column"] + 1000)
            assert np.array_equal(got[:, 2], c.hits["num_match"]), what
            return c
        kernels = set()
        for segs in (1, 3):
            with ctx.tuning(force_segs=segs):
                for k, t in ((1, 0.0), (64, 0.5), (1024, 0.0), (1024, 0.8), (5, 1.0)):
                    kernels.add(both(k, t, "sparse segs=%d" % segs).search_kernel.split("<")[0])
        assert kernels == {"topk_tile_kernel", "count_kernel"}, kernels
        for call in (lambda: ka.search_topk(sp, other, 10, 0.5),
                     lambda: ka.search_topk_device_append(sp, other, 10, hits, count, threshold=0.5)):
            with pytest.raises(ka.KwageError) as ei:
                call()
            assert ei.value.code == -6 and "not among the rows" in str(ei.value), ei.value
        both(64, 0.5, "sparse after the refused batch")                 # still gives the right lists
    finally:
        other.close()
        b.close()
        full.close()
        sp.close()


# ---- 7. the k-mer layout shared with kwage_search ------------------------------------------------------------------------
def test_kmer_layout_shared_with_threshold_search(ka, ctx, oracle):
    """A batch's k-mer layout is built by whichever search comes first and reused by the other kind: a top-k search
    first must leave kwage_search the lists of a fresh batch, in every family, and the other way round."""
    rng = np.random.default_rng(5)
    kmer, nh, L, nf = 31, 2, 12, 20000
    genome = rand_seq(rng, 6000)
    grow = oracle.row_indices(oracle.unique_kmers(genome, kmer), kmer, nh, L).reshape(-1)
    bits = rand_bits(rng, (1 << L, nf), 0.8)
    for c in (3, 9000, 19999):
        bits[grow, c] = True
    g, files, span = add_files(ka, ctx, kmer, nh, L, [(pack_columns(bits, rng), nf, None)])
    queries = [genome[:150], genome[700:850], rand_seq(rng, 150),
               genome[1000:1000 + 1500 + kmer - 1],            # > 1024 positions, one workgroup's table
               genome[:2049 + kmer - 1],                        # > 2048 positions: the global distinct set, three chunks
               "ACGTAC", genome[3000:3000 + 2900 + kmer - 1]]
    per_query = reference(oracle, files, span, kmer, nh, L, queries)
    walk = dict(walk_min_rows=1, count_walk_min_rows=1, walk_waves=23, count_walk_waves=23)

    def threshold_searches(b):
        out = []
        for knobs in ({}, walk):
            with ctx.tuning(**knobs):
                for t in (1.0, 0.8, 0.3):
                    for flags in (0, ka.SEARCH_EARLY_EXIT):
                        r = g.search(b, t, flags)
                        out.append((r.search_kernel, r.hits, r.num_query_kmer, r.query_threshold))
        return out

    def topk_searches(b):
        out = []
        for segs in (1, 3):
            with ctx.tuning(force_segs=segs):
                for k, t in ((1, 0.0), (64, 0.5), (1024, 0.8)):
                    r = check(ka, oracle, g, b, per_query, k, t, "layout segs=%d" % segs)
                    out.append((r.search_kernel, r.hits, r.num_query_kmer, r.query_threshold))
        return out

    def same(x, y):
        assert len(x) == len(y)
        for a, c in zip(x, y):
            assert a[0] == c[0] and all(np.array_equal(u, v) for u, v in zip(a[1:], c[1:])), (a[0], c[0])

    bs = [ka.Batch(ctx, queries) for _ in range(4)]
    try:
        first_topk = ka.search_topk(g, bs[0], 64, 0.5)            # batch A: the top-k search builds the layout
        a = threshold_searches(bs[0])
        fresh = threshold_searches(bs[1])                          # batch B: kwage_search builds it
        same(a, fresh)
        kinds = {name.split("<")[0] for name, *_ in fresh}
        assert {"and_kernel", "and_walk_kernel", "count_kernel", "count_walk_kernel"} <= kinds, kinds
        assert_hits_equal(first_topk.hits, expected_hits(oracle, per_query, 0.5, 64)[0], "layout: first top-k")
        g.search(bs[2], 0.8)                                       # batch C: a threshold search first, then top-k
        same(topk_searches(bs[2]), topk_searches(bs[3]))           # batch D: top-k fresh
    finally:
        for b in bs:
            b.close()
        g.close()
