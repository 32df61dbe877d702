"""kwage_search_presence at every shape the library can launch (tests/presence_shapes.py): every counter width (7 / 10 /
14 / 20 / 32 planes) and hash count of presence_tile_kernel, every width of presence_combine_kernel behind forced
segments, presence_and_kernel at one to five hash functions -- on a narrow group of two tiles whose last one the span
cuts, with and without the early exit; and a batch of long queries that the slab of the segments' partial counters
cuts into slices.

Expected bitmap: `count >= floor` on the real columns, the floor the oracle's (oracle.query_threshold), the counts the
device's threshold search at a threshold whose floor is 0 (it lists every real column of every query with k-mers;
itself pinned to the oracle by the parity suite), and for the widths up to 14 planes the CPU oracle's counts as well.
The threshold below 1 is chosen per batch so that about half of the longest query's columns pass.  Every case asserts
the exact kernel name it meant to reach (tests/test_presence_isa.py checks that the names cover what the compiler
emitted)."""
import numpy as np
import pytest

import presence_shapes as ps
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
    rng = np.random.default_rng(2 ** 20 + 1)
    genome = rand_seq(rng, max(ps.POSITIONS.values()) + KMER - 1)
    out = {}
    for p, positions in ps.POSITIONS.items():
        queries = [rand_seq(rng, 120), genome[:positions + KMER - 1], "ACG", genome[500:500 + min(positions, 700) // 2 + KMER - 1]]
        out[p] = (queries, ka.Batch(ctx, queries))
    yield out
    for _, b in out.values():
        b.close()


def from_threshold_search(res, n, span):
    m = np.full((n, span), -1, dtype=np.int64)
    m[res.hits["query"], res.hits["column"]] = res.hits["num_match"]
    return m


def expected_bitmap(oracle, counts, nk, t):
    """counts: int64 [n, span], -1 where a column is not real (or the query has no k-mers)."""
    floors = np.array([oracle.query_threshold(float(np.float32(t)), int(n)) for n in nk], dtype=np.int64)
    return (counts >= floors[:, None]) & (counts >= 0)


@pytest.mark.parametrize("nh", ps.HASHES)
def test_every_presence_kernel_shape(ka, ctx, oracle, batches, nh):
    rng = np.random.default_rng(400 + nh)
    density = (0.5, 0.7, 0.78, 0.82, 0.85)[nh - 1]
    images = []
    for nf in (120, 8300 - 37):                          # two files: 8383 columns behind a pad, two tiles, the last cut by the span
        bits = rand_bits(rng, (1 << L, nf), density)
        bits[:, [4, nf - 1]] = True                      # every row: the count n sets the top plane bit and passes at t = 1
        bits[: (1 << L) // 2, 9] = True
        images.append((pack_columns(bits, rng), nf))
    g = ka.Group(ctx, KMER, nh, L, sum(nf + 128 for _, nf in images))
    files = [(g.add_columns(img, nf), img, nf, None) for img, nf in images]
    g.finalize()
    span = g.column_span
    assert span > 8192 and span % 128 != 0 and span < g.row_stride * 8
    reached = set()
    try:
        for p in ps.PLANES:
            queries, b = batches[p]
            positions = ps.POSITIONS[p]
            with ctx.tuning(count_walk=0):
                res0 = g.search(b, FLOOR_ZERO)
            counts = from_threshold_search(res0, len(queries), span)
            nk = res0.num_query_kmer
            assert nk[1] == positions and nk[2] == 0 and ps.planes_for(positions) == p
            assert counts[1].max() == positions and (counts[2] == -1).all()
            if p <= 14:
                for q, seq in enumerate(queries):
                    c = column_counts(oracle, files, span, KMER, nh, L, oracle.unique_kmers(seq, KMER))
                    assert np.array_equal(counts[q], c if nk[q] else np.full(span, -1)), (p, q)
            real = counts[1] >= 0
            t_half = float(np.float32(np.median(counts[1][real]) / positions))
            assert 0 < t_half < 1
            for t in (t_half, 1.0):
                exp = expected_bitmap(oracle, counts, nk, t)
                assert exp[1].any() and not exp[1][real].all() and not exp[2].any()
                if t == t_half:
                    assert exp[1].sum() > real.sum() // 4
                for segs in (1, ps.FORCED_SEGS):
                    name = ps.combine_name(p, nh, positions) if segs != 1 else (ps.AND_NAME if t == 1.0 else ps.tile_name(p, nh))
                    for flags in (0, ka.SEARCH_EARLY_EXIT):
                        with ctx.tuning(force_segs=segs):
                            res = ka.search_presence(g, b, t, flags)
                        assert res.kernel == name, (res.kernel, name)
                        assert np.array_equal(res.num_query_kmer, nk)
                        got = res.unpack()
                        bad = np.argwhere(got != exp)
                        assert bad.size == 0, (name, t, flags, bad[:5].tolist())
                        assert np.array_equal(res.passing, exp.sum(axis=1))
                    reached.add(("presence_combine_kernel", (p,)) if segs != 1 else ("presence_and_kernel", ()) if t == 1.0 else ("presence_tile_kernel", (p, nh)))
        assert reached == {s for s in ps.TILE_SHAPES if s[1][1] == nh} | set(ps.COMBINE_SHAPES) | {("presence_and_kernel", ())}
    finally:
        g.close()


def test_default_dispatch_picks_the_unsegmented_forms_for_many_reads(ka, ctx, oracle):
    """2048 (query, tile) pairs and more: no segments by the rule itself (the tile kernel, the AND kernel at t = 1);
    fewer: segments."""
    rng = np.random.default_rng(9)
    g = ka.Group(ctx, KMER, 2, L, 8192 * 2)
    g.add_random_columns(8192 * 2 - 40, 11, 100)
    g.finalize()
    genome = rand_seq(rng, 5000)
    many = ka.Batch(ctx, [genome[i:i + 150] for i in range(0, 2200 * 2, 2)][:1100])
    few = ka.Batch(ctx, [genome[:1500], genome[100:900]])
    try:
        for b, t, name in ((many, 0.3, ps.tile_name(7, 2)), (many, 1.0, ps.AND_NAME), (few, 0.3, "+presence_combine_kernel<14>"), (few, 1.0, "+presence_combine_kernel<14>")):
            with ctx.tuning(count_walk=0):
                res0 = g.search(b, FLOOR_ZERO)
            exp = expected_bitmap(oracle, from_threshold_search(res0, b.n, g.column_span), res0.num_query_kmer, t)
            for flags in (0, ka.SEARCH_EARLY_EXIT):
                res = ka.search_presence(g, b, t, flags)
                assert name in res.kernel, res.kernel
                assert np.array_equal(res.unpack(), exp), (name, t, flags)
    finally:
        many.close()
        few.close()
        g.close()


def test_presence_sliced_slab_bound(ka, ctx, oracle):
    """test_gpu_scores_shapes.py's test_score_matrix_sliced_slab_bound for the presence search: long queries over
    ~350 000 columns with 1024 forced segments, so that the 1 GiB slab of partial counters holds three of the eight
    queries: slices (3, 3, 2), a query without k-mers (a zero row) in the second and in the last.  Every bit against the
    oracle's counts and floors."""
    import torch
    from kwage_amd.native import lib, check
    rng = np.random.default_rng(41)
    nh, L8, B = 1, 8, 5003
    base = rand_bits(rng, (1 << L8, B), 0.5)
    base[:, 77] = True                                            # every row: the count n, copied into every tile
    g = ka.Group(ctx, KMER, nh, L8, sum((nf + 127) // 128 * 128 for nf in (100003, 90000, 85007, 75000)))
    files = []
    for nf, shift in ((100003, 0), (90000, 3), (85007, 9), (75000, 2500)):      # column j a copy of base column (7 j + shift) % B
        cmap = (np.arange(nf, dtype=np.int64) * 7 + shift) % B
        base_img = pack_columns(base, rng)
        files.append((g.add_columns(pack_columns(base[:, cmap], rng), nf), base_img, nf, cmap))
    g.finalize()
    span, w = g.column_span, (g.row_bytes + 15) // 16 * 16
    genome = rand_seq(rng, 72000)
    P = (70000, 64000, 52000, 50000, 0, 41000, 30000, 0)
    queries = [genome[i * 100:i * 100 + p + KMER - 1] if p else "ACGT" for i, p in enumerate(P)]
    segs = 1024
    seg_kmers = -(-max(P) // segs)
    assert seg_kmers == 69 and ps.planes_for(seg_kmers) == 7 and ps.planes_for(max(P)) == 20
    slab_q = (1 << 30) // (-(-max(P) // seg_kmers) * ps.planes_for(seg_kmers) * g.row_stride)
    assert slab_q == 3, slab_q                                     # slices (3, 3, 2): a zero row in the second and the last
    n = len(queries)
    counts = np.full((n, span), -1, dtype=np.int64)
    nk = np.zeros(n, dtype=np.uint32)
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, KMER)
        nk[q] = len(kmers)
        if len(kmers):
            counts[q] = column_counts(oracle, files, span, KMER, nh, L8, kmers)
    assert nk.tolist() == list(P) and counts[0].max() == P[0]
    t_half = float(np.float32(np.median(counts[0][counts[0] >= 0]) / P[0]))
    b = ka.Batch(ctx, queries)
    try:
        for t in (t_half, 1.0):
            exp = expected_bitmap(oracle, counts, nk, t)
            assert exp[0].any() and not exp[4].any() and not exp[7].any()
            with ctx.tuning(force_segs=segs):
                # device form: rows 32 bytes longer than what is written
                out = torch.full((n, w + 32), 0xA5, dtype=torch.uint8, device="cuda:0")
                pas = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                res = ka.search_presence_device(g, b, t, out, pas)
                assert res.kernel == "count_kernel<7,1>+presence_combine_kernel<20>", res.kernel
                got = out.cpu().numpy()
                assert (got[:, w:] == 0xA5).all(), t
                bits = np.unpackbits(np.ascontiguousarray(got[:, :w]), axis=1, bitorder="little")[:, :span].astype(bool)
                bad = np.argwhere(bits != exp)
                assert bad.size == 0, (t, bad[:5].tolist())
                assert np.array_equal(pas.cpu().numpy().view(np.uint32), exp.sum(axis=1)), t
                # host form: the same slices, then the strided copy
                host = np.full((n, w + 16), 0xA5, dtype=np.uint8)
                hnk = np.zeros(n, dtype=np.uint32)
                check(lib().kwage_search_presence(g._h, b._h, float(t), host.ctypes.data, w + 16, None, hnk.ctypes.data, 0, None))
                assert (host[:, w:] == 0xA5).all() and np.array_equal(host[:, :w], got[:, :w]), t
                assert np.array_equal(hnk, nk), t
    finally:
        b.close()
        g.close()
