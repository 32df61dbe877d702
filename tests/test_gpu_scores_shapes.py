"""kwage_search_scores at every shape the library can launch (tests/scores_shapes.py): every counter width (7 / 10 / 14 /
20 / 32 planes) and hash count of score_tile_kernel, every width of score_combine_kernel behind forced segments, both
store epilogues of each -- on a narrow group of two tiles whose last one the span cuts; and a batch of long queries
that the slab of the segments' partial counters cuts into slices.

Expected matrix: the device's threshold search at a threshold whose floor is 0 (it lists every real column of every
query with k-mers; itself pinned to the oracle by the parity suite), and for the widths up to 14 planes the CPU
oracle's counts as well.  Every case asserts the exact kernel name it meant to reach (tests/test_scores_isa.py checks
that the names cover what the compiler emitted)."""
import numpy as np
import pytest

import scores_shapes as ss
from topk_reference import column_counts, pack_columns, rand_bits, rand_seq

pytestmark = pytest.mark.gpu

KMER, L = 31, 10
FLOOR_ZERO = 1e-9              # (unsigned)(t * n) == 0 for every n < 2^29


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


@pytest.fixture(scope="module")
def batches(ka, ctx):
    """Per counter width: (queries, batch) -- the longest query reaches the width, one query has no k-mers."""
    rng = np.random.default_rng(2 ** 20)
    genome = rand_seq(rng, max(ss.POSITIONS.values()) + KMER - 1)
    out = {}
    for p, positions in ss.POSITIONS.items():
        queries = [rand_seq(rng, 120), genome[:positions + KMER - 1], "ACG", genome[500:500 + min(positions, 700) // 2 + KMER - 1]]
        out[p] = (queries, ka.Batch(ctx, queries))
    yield out
    for _, b in out.values():
        b.close()


def from_threshold_search(res, n, span):
    m = np.zeros((n, span), dtype=np.uint32)
    m[res.hits["query"], res.hits["column"]] = res.hits["num_match"]
    return m


@pytest.mark.parametrize("nh", ss.HASHES)
def test_every_score_kernel_shape(ka, ctx, oracle, batches, nh):
    rng = np.random.default_rng(300 + nh)
    density = (0.5, 0.7, 0.78, 0.82, 0.85)[nh - 1]
    images = []
    for nf in (120, 8300 - 37):                          # two files: 8383 columns behind a pad, two tiles, the last cut by the span
        bits = rand_bits(rng, (1 << L, nf), density)
        bits[:, [4, nf - 1]] = True                      # every row: the score n sets the top plane bit
        bits[: (1 << L) // 2, 9] = True
        images.append((pack_columns(bits, rng), nf))
    g = ka.Group(ctx, KMER, nh, L, sum(nf + 128 for _, nf in images))
    files = [(g.add_columns(img, nf), img, nf, None) for img, nf in images]
    g.finalize()
    span = g.column_span
    assert span > 8192 and span % 128 != 0 and span < g.row_stride * 8
    reached = set()
    try:
        for p in ss.PLANES:
            queries, b = batches[p]
            positions = ss.POSITIONS[p]
            with ctx.tuning(count_walk=0):
                exp = from_threshold_search(g.search(b, FLOOR_ZERO), len(queries), span)
            nk = g.search(b, 0.5).num_query_kmer
            assert nk[1] == positions and nk[2] == 0 and ss.planes_for(positions) == p
            assert exp[1].max() == positions and not exp[2].any()
            if p <= 14:
                for q, seq in enumerate(queries):
                    counts = column_counts(oracle, files, span, KMER, nh, L, oracle.unique_kmers(seq, KMER))
                    assert np.array_equal(exp[q], np.maximum(counts, 0) if nk[q] else np.zeros(span)), (p, q)
            for segs, name in ((1, ss.tile_name(p, nh)), (ss.FORCED_SEGS, ss.combine_name(p, nh, positions))):
                for form in (0, 1):
                    with ctx.tuning(force_segs=segs, scores_form=form):
                        res = ka.search_scores(g, b)
                    assert res.kernel == name, (res.kernel, name)
                    assert np.array_equal(res.num_query_kmer, nk)
                    bad = np.argwhere(res.scores != exp)
                    assert bad.size == 0, (name, form, bad[:5].tolist(), [(int(res.scores[q, c]), int(exp[q, c])) for q, c in bad[:5]])
                reached.add(("score_tile_kernel", (p, nh)) if segs == 1 else ("score_combine_kernel", (p,)))
        assert reached == {s for s in ss.TILE_SHAPES if s[1][1] == nh} | set(ss.COMBINE_SHAPES)
    finally:
        g.close()


def test_default_dispatch_picks_the_tile_form_for_many_reads(ka, ctx):
    """2048 (query, tile) pairs and more: no segments by the rule itself; fewer: segments."""
    rng = np.random.default_rng(8)
    g = ka.Group(ctx, KMER, 2, L, 8192 * 2)
    g.add_random_columns(8192 * 2 - 40, 11, 100)
    g.finalize()
    genome = rand_seq(rng, 5000)
    many = ka.Batch(ctx, [genome[i:i + 150] for i in range(0, 2200 * 2, 2)][:1100])
    few = ka.Batch(ctx, [genome[:1500], genome[100:900]])
    try:
        for b, name in ((many, ss.tile_name(7, 2)), (few, "+score_combine_kernel<14>")):
            res = ka.search_scores(g, b)
            assert name in res.kernel, res.kernel
            with ctx.tuning(count_walk=0):
                exp = from_threshold_search(g.search(b, FLOOR_ZERO), b.n, g.column_span)
            assert np.array_equal(res.scores, exp)
    finally:
        many.close()
        few.close()
        g.close()


def test_score_matrix_sliced_slab_bound(ka, ctx, oracle):
    """test_gpu_topk_shapes.py's test_sliced_batch_slab_bound for the score search: long queries over ~350 000 columns
    with 1024 forced segments, so that the 1 GiB slab of partial counters holds three of the eight queries: slices
    (3, 3, 2), a query without k-mers (a zero row) in the second and in the last.  Every cell against the oracle."""
    import torch
    from kwage_amd.native import lib, check
    rng = np.random.default_rng(41)
    nh, L8, B, sentinel = 1, 8, 5003, -1234567
    base = rand_bits(rng, (1 << L8, B), 0.5)
    base[:, 77] = True                                            # every row: the score n, copied into every tile
    g = ka.Group(ctx, KMER, nh, L8, sum((nf + 127) // 128 * 128 for nf in (100003, 90000, 85007, 75000)))
    files = []
    for nf, shift in ((100003, 0), (90000, 3), (85007, 9), (75000, 2500)):      # column j a copy of base column (7 j + shift) % B
        cmap = (np.arange(nf, dtype=np.int64) * 7 + shift) % B
        base_img = pack_columns(base, rng)
        files.append((g.add_columns(pack_columns(base[:, cmap], rng), nf), base_img, nf, cmap))
    g.finalize()
    span = g.column_span
    genome = rand_seq(rng, 72000)
    P = (70000, 64000, 52000, 50000, 0, 41000, 30000, 0)
    queries = [genome[i * 100:i * 100 + p + KMER - 1] if p else "ACGT" for i, p in enumerate(P)]
    segs = 1024
    seg_kmers = -(-max(P) // segs)
    assert seg_kmers == 69 and ss.planes_for(seg_kmers) == 7 and ss.planes_for(max(P)) == 20
    slab_q = (1 << 30) // (-(-max(P) // seg_kmers) * ss.planes_for(seg_kmers) * g.row_stride)
    assert slab_q == 3, slab_q                                     # slices (3, 3, 2): a zero row in the second and the last
    n = len(queries)
    exp = np.zeros((n, span), dtype=np.uint32)
    nk = np.zeros(n, dtype=np.uint32)
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, KMER)
        nk[q] = len(kmers)
        if len(kmers):
            exp[q] = np.maximum(column_counts(oracle, files, span, KMER, nh, L8, kmers), 0)
    assert nk.tolist() == list(P) and exp[0].max() == P[0] and not exp[4].any() and not exp[7].any()
    b = ka.Batch(ctx, queries)
    try:
        for form in (0, 1):
            with ctx.tuning(force_segs=segs, scores_form=form):
                # device form: a matrix 12 cells wider than the span
                out = torch.full((n, span + 12), sentinel, dtype=torch.int32, device="cuda:0")
                nkd = torch.full((n,), sentinel, dtype=torch.int32, device="cuda:0")
                res = ka.search_scores_device(g, b, out, nkd)
                assert res.kernel == "count_kernel<7,1>+score_combine_kernel<20>", res.kernel
                got = out.cpu().numpy()
                assert (got[:, span:] == sentinel).all(), form
                bad = np.argwhere(got[:, :span].view(np.uint32) != exp)
                assert bad.size == 0, (form, bad[:5].tolist(), [(int(got[q, c]), int(exp[q, c])) for q, c in bad[:5]])
                assert np.array_equal(nkd.cpu().numpy().view(np.uint32), nk), form
                # host form: the same slices, then the strided copy
                host = np.full((n, span + 4), sentinel, dtype=np.int32)
                hnk = np.zeros(n, dtype=np.uint32)
                check(lib().kwage_search_scores(g._h, b._h, host.ctypes.data, span + 4, hnk.ctypes.data, 0, None))
                assert (host[:, span:] == sentinel).all() and np.array_equal(host[:, :span].view(np.uint32), exp), form
                assert np.array_equal(hnk, nk), form
    finally:
        b.close()
        g.close()
