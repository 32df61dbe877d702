"""kwage_search_topk (the top-k search) through the C ABI and the Python mirror, against the CPU oracle.

Expected lists: the oracle's count of every column (a threshold whose floor is 0), then the contract of
include/kwage_amd.h -- floor f = (unsigned)(t * n), eligible = real columns with count >= f, key (count descending,
column ascending), cut at k.  The device's own threshold search (kwage_search at the same t, cut by the same rule) is
a second oracle."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def _floor(t, n):
    from kwage_amd.native import lib
    import ctypes as C
    return int(lib().kwage_query_threshold(C.c_float(t), n))


def _expected(counts, valid_cols, t, n, k):
    """counts: {column: count} over every real column; the contract's selection, returned ordered by column."""
    if n == 0:
        return []
    f = _floor(t, n)
    elig = [(c, m) for c, m in ((c, counts.get(c, 0)) for c in valid_cols) if m >= f]
    elig.sort(key=lambda cm: (-cm[1], cm[0]))
    return sorted(elig[:k])


def _make_group(ka, ctx, rng, k, num_hash, L, files_nf, density, dup_pairs):
    """A group of several 'files' (add_columns), garbage in the pad bits of every image, planted duplicate columns.
    Returns (group, [(first_column, image, nf)])."""
    g = ka.Group(ctx, k, num_hash, L, sum(nf + 128 for nf in files_nf))
    files = []
    for nf in files_nf:
        bits = rng.random((1 << L, nf)) < density
        for a, b in dup_pairs:                        # equal columns: ties that straddle the cut
            if a < nf and b < nf:
                bits[:, b] = bits[:, a]
        width = (nf + 7) // 8 + 3
        img = np.zeros((1 << L, width * 8), dtype=bool)
        img[:, :nf] = bits
        img[:, nf:] = rng.random((1 << L, width * 8 - nf)) < 0.5      # pad bits: garbage
        packed = np.packbits(img, axis=1, bitorder="little")
        first = g.add_columns(packed, nf)
        files.append((first, np.ascontiguousarray(packed), nf))
    g.finalize()
    return g, files


def _oracle_counts(oracle, files, k, num_hash, L, kmers):
    counts, valid = {}, []
    for first, img, nf in files:
        hits, _ = oracle.search_image(img, img.shape[1], k, num_hash, L, nf, kmers, 1e-12)
        for c, m in hits:
            counts[first + c] = m
        valid.extend(range(first, first + nf))
    return counts, valid


@pytest.mark.parametrize("num_hash", [1, 3])
def test_topk_matches_oracle_and_threshold_search(ka, ctx, oracle, num_hash):
    from kwage_amd import native
    rng = np.random.default_rng(7 + num_hash)
    kmer, L = 21, 11
    density = 0.35 if num_hash == 1 else 0.7
    dup_pairs = [(3, 4), (3, 900), (17, 2000), (100, 101), (100, 102), (5000, 5001)]
    g, files = _make_group(ka, ctx, rng, kmer, num_hash, L, [3001, 9000 - 333], density, dup_pairs)
    genome = "".join(rng.choice(list("ACGT"), size=120000))
    queries = [genome[i * 700:i * 700 + ln] for i, ln in enumerate((100, 150, 333, 1000, 640))]
    queries += ["ACGTACGTAC",                                    # shorter than k: no k-mers
                genome[:100000]]                                  # long: the segmented path
    counts = []
    for q in queries:
        kmers = oracle.unique_kmers(q, kmer)
        counts.append((len(kmers),) + _oracle_counts(oracle, files, kmer, num_hash, L, kmers))
    b = ka.Batch(ctx, queries)
    try:
        for t in (0.0, 0.5, 0.8, 1.0):
            thr = None
            if t > 0:
                thr = g.search(b, t).per_query()
            # default: this small batch (fewer than 2048 tiles) takes the segmented form; force_segs=1: one wave per
            # (query, 8192-column tile) -- topk_tile_kernel, several queries x two tiles
            for segs, kernel in ((0, "topk_combine_kernel"), (1, "topk_tile_kernel")):
                with ctx.tuning(force_segs=segs):
                    for kk in (1, 7, 64, native.TOPK_MAX):
                        res = ka.search_topk(g, b, kk, t, ka.SEARCH_TIMING)
                        assert res.search_kernel_launches >= 1 and kernel in res.search_kernel, (segs, res.search_kernel)
                        per_q = res.per_query()
                        for i, (n, cnt, valid) in enumerate(counts):
                            assert res.num_query_kmer[i] == n
                            assert res.query_threshold[i] == _floor(t, n)
                            exp = _expected(cnt, valid, t, n, kk)
                            assert per_q[i] == exp, (num_hash, t, segs, kk, i, per_q[i][:6], exp[:6])
                            if thr is not None:
                                alt = sorted(sorted(thr[i], key=lambda cm: (-cm[1], cm[0]))[:kk])
                                assert per_q[i] == alt, (num_hash, t, segs, kk, i)
        # the segmented form on every query (forced) gives the same lists
        with ctx.tuning(force_segs=3):
            res = ka.search_topk(g, b, 64, 0.5)
            assert "topk_combine_kernel" in res.search_kernel, res.search_kernel
            for i, (n, cnt, valid) in enumerate(counts):
                assert res.per_query()[i] == _expected(cnt, valid, 0.5, n, 64), i
    finally:
        b.close()
        g.close()


def test_topk_ties_straddle_the_cut(ka, ctx, oracle):
    """Many equal scores around row k: the lowest columns of the tied run are taken, across tiles of 8192 columns."""
    rng = np.random.default_rng(11)
    kmer, L, nf = 21, 10, 20000
    g = ka.Group(ctx, kmer, 1, L, nf)
    bits = np.zeros((1 << L, nf), dtype=bool)
    q = "".join(rng.choice(list("ACGT"), size=300))
    b = ka.Batch(ctx, [q])
    _, rows = ka.hash_batch(ctx, kmer, 1, L, b)
    r = rows[0].reshape(-1)
    tied = [5, 77, 8191, 8192, 9000, 16383, 16384, 19999]       # columns with the same full score, in three tiles
    for c in tied:
        bits[r, c] = True
    bits[r[: len(r) // 2], 12345] = True                        # a lower score
    packed = np.packbits(bits, axis=1, bitorder="little")
    g.add_columns(packed, nf)
    g.finalize()
    n = len(oracle.unique_kmers(q, kmer))
    cnt, valid = _oracle_counts(oracle, [(0, np.ascontiguousarray(packed), nf)], kmer, 1, L, oracle.unique_kmers(q, kmer))
    assert all(cnt[c] == n for c in tied)
    try:
        for segs, kernel in ((0, "topk_combine_kernel"), (1, "topk_tile_kernel")):
            with ctx.tuning(force_segs=segs):
                for kk, t in ((1, 0.0), (3, 0.0), (5, 1.0), (8, 0.5), (9, 0.0), (9, 0.9), (40, 0.0)):
                    res = ka.search_topk(g, b, kk, t)
                    assert kernel in res.search_kernel, (segs, res.search_kernel)
                    got = res.per_query()[0]
                    exp = _expected(cnt, valid, t, n, kk)
                    assert got == exp, (segs, kk, t, got)
                    if kk <= len(tied):
                        assert got == [(c, n) for c in tied[:kk]], (segs, kk, t, got)
    finally:
        b.close()
        g.close()


def test_topk_tile_kernel_many_queries(ka, ctx, oracle):
    """Enough (query, tile) pairs that the library picks topk_tile_kernel by itself: 1001 reads over three 8192-column
    tiles (3003 tiles -- not a multiple of the four waves of a workgroup), ties planted across the tiles."""
    rng = np.random.default_rng(23)
    kmer, L = 21, 10
    dup_pairs = [(1, 8200), (1, 16500), (40, 41), (8191, 8192)]
    g, files = _make_group(ka, ctx, rng, kmer, 1, L, [20000 - 5], 0.3, dup_pairs)
    genome = "".join(rng.choice(list("ACGT"), size=40000))
    queries = [genome[(i * 37) % 39000:(i * 37) % 39000 + 150] for i in range(1001)]
    check = list(range(0, 1001, 97)) + [1000]
    counts = {i: (len(oracle.unique_kmers(queries[i], kmer)),) +
              _oracle_counts(oracle, files, kmer, 1, L, oracle.unique_kmers(queries[i], kmer)) for i in check}
    b = ka.Batch(ctx, queries)
    try:
        for kk, t in ((1, 0.0), (10, 0.0), (64, 0.5), (ka.TOPK_MAX, 0.8)):
            res = ka.search_topk(g, b, kk, t)
            assert "topk_tile_kernel" in res.search_kernel, res.search_kernel
            per_q = res.per_query()
            for i, (n, cnt, valid) in counts.items():
                assert per_q[i] == _expected(cnt, valid, t, n, kk), (kk, t, i)
    finally:
        b.close()
        g.close()


def test_topk_argument_errors(ka, ctx):
    from kwage_amd import native
    g = ka.Group(ctx, 21, 1, 8, 100)
    g.add_random_columns(100, 3, 64)
    g.finalize()
    b = ka.Batch(ctx, ["ACGT" * 20])
    try:
        for kk, t in ((0, 0.5), (native.TOPK_MAX + 1, 0.5), (5, -0.1), (5, 1.5), (5, math.nan)):
            with pytest.raises(native.KwageError) as e:
                ka.search_topk(g, b, kk, t)
            assert e.value.code == -1, (kk, t)
        assert ka.search_topk(g, b, native.TOPK_MAX, 0.0).hits.size == 100
    finally:
        b.close()
        g.close()
