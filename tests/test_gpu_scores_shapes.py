"""kwage_search_scores at every shape the library can launch (tests/scores_shapes.py): every counter width (7 / 10 / 14 /
20 / 32 planes) and hash count of score_tile_kernel, every width of score_combine_kernel behind forced segments, both
store epilogues of each -- on a narrow group of two tiles whose last one the span cuts.

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
