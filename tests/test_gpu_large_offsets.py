"""The searches and the live insert where 32-bit arithmetic would go wrong, and the insert's staged chunks.

1. Four resident groups of 6 GiB, one per row-width class of the kernel table (GROUPS): a third of their rows start at or
   beyond byte 2^32.  Background columns are random (add_random_columns); seven KNOWN filters -- three genomes, all ones,
   empty, two at density 1/2 -- are live-inserted behind them after finalize.  No host copy of such a matrix exists:
   expected values are large_shapes.py's, from the rows a batch addresses (Group.read_rows, itself checked against the
   known filters at sampled rows on both sides of byte 2^32) and from the known filters' own bits.
2. Results beyond byte 2^32: the device forms of the score and presence searches into tensors of 4.3 GB.
3. kwage_group_insert_filters / _bloom_files with more than 64 MiB of filters per call: insert.hip insert_from_host stages
   such a call in chunks of rows, and every chunk but the first has a row base and a source offset.

Every comparison is exact equality, and every test asserts the premise it exists for (offsets beyond 2^32 addressed,
results above 2^32 bytes, staging above 64 MiB).

Two things the library decides, met while building the groups:
  - the first insert behind another block starts on the next 16-byte boundary of the row (insert_plan.hpp plan_insert), so
    the head-room of a group filled to within fewer than 128 columns of its capacity takes no insert: the groups here are
    filled up to 128 columns short of their capacity;
  - kwage_group_add_columns refuses a finalized group, so the bytes between row_bytes and the stride cannot be made
    visible there by one-column blocks (test_gpu_live_insert.py's method): that check runs on the un-finalized groups of
    part 3, behind inserts that were staged in chunks."""
import time

import numpy as np
import pytest

import large_shapes as ls
import search_shapes as ss
from topk_reference import assert_hits_equal, column_counts, pack_columns, rand_bits

pytestmark = pytest.mark.gpu

K = 31
GIB = 1 << 30
HEADROOM = 128                # columns left free behind the background: 16 bytes of a row, the least an insert can take
# key: (log_2_filter_len, row stride in bytes, num_hash, how often the batch is repeated)
GROUPS = {"narrow": (24, 384, 1, 6),         # several queries per wave (rows <= 512 B): those forms want 64 queries and more
          "tile": (22, 1536, 3, 1),          # KiB-tile kernels, screen + refine
          "walk": (20, 6144, 2, 1),          # walk, band walk, count walk (rows of 2-16 KiB)
          "wide": (18, 24576, 5, 1)}         # the wide tiled shape (rows above 16 KiB)
KEYS = list(GROUPS)
ONES, EMPTY, RETIRED = 3, 4, 3               # known filters: 0-2 genomes, 3 all ones, 4 empty, 5-6 random
EE = 1
# (family, threshold, flags, knobs): the persistent and early-exit forms a group's width admits, forced as search_shapes.py does
AND_SCREEN = ("and_screen_kernel", 1.0, EE, {})
COUNT_SCREEN = ("count_screen_kernel", 0.8, EE, ss.SCREEN)
COUNT_WALK = ("count_walk_kernel", 0.8, 0, ss.PF)
WHOLE = dict(force_segs=1)    # whole row lists: the tiled kernels themselves, not segments and a combine pass (the batch's long query is segmented by default)
TILED = [("and_kernel", 1.0, 0, dict(WHOLE, walk=0)), ("count_kernel", 0.8, 0, WHOLE)]
FORMS = {"narrow": [("and_narrow_kernel", 1.0, 0, WHOLE), ("count_narrow_kernel", 0.8, 0, WHOLE)],
         "tile": TILED + [("and_walk_kernel", 1.0, 0, ss.WALK), AND_SCREEN, COUNT_WALK, COUNT_SCREEN],
         "walk": TILED + [("and_walk_kernel", 1.0, 0, ss.WALK), ("and_band_walk_kernel", 1.0, 0, ss.BAND), AND_SCREEN, COUNT_WALK, COUNT_SCREEN],
         "wide": TILED + [AND_SCREEN, COUNT_WALK, COUNT_SCREEN]}


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def env(ka, oracle):
    e = Env(ka, oracle)
    yield e
    e.close()


class Env:
    """The module's context, groups and batches, built on first use and shared by the tests."""

    def __init__(self, ka, oracle):
        self.ka, self.oracle = ka, oracle
        self.ctx = ka.Context(0)
        free, _ = self.ctx.mem_info()
        if free < 32 * GIB:
            self.ctx.close()
            pytest.skip("needs 32 GiB of free HBM")
        import torch
        torch.zeros(1, device="cuda:%d" % self.ctx.device)      # (torch's start-up: once, here)
        self.groups, self.shallow_group = {}, None
        rng = np.random.default_rng(2032)
        g0, g1, g2 = self.genomes = [ls.random_dna(rng, 3600) for _ in range(3)]
        self.queries = [g0[100:250], g1[500:650], g2[200:3230],                       # reads and a query of 3000 positions: 14-plane counters
                        ls.mutated(g0[100:250], 41), ls.mutated(g1[1000:1400], 97),   # counts between the floor and n
                        ls.random_dna(rng, 150), ls.random_dna(rng, 150),
                        "", g0[300:300 + K], g1[2000:2060] + "N" + g1[2061:2130], g1[500:650], ls.random_dna(rng, 200)]
        self.from_genome = {0: 0, 1: 1, 2: 2, 8: 0, 9: 1, 10: 1}                      # query -> the genome it is cut from

    def close(self):
        for b in self.groups.values():
            b.close()
        if self.shallow_group is not None:
            self.shallow_group[0].close()
        self.ctx.close()

    def group(self, key):
        if key not in self.groups:
            self.groups[key] = Big(self, key)
        return self.groups[key]

    def shallow(self):
        """A wide, shallow group as test_gpu_scores_shapes.py builds it: ~350 000 columns that are copies of 5003 base
        columns, 2^8 rows -- cheap for the oracle."""
        if self.shallow_group is None:
            rng = np.random.default_rng(41)
            B, L8 = 5003, 8
            base = rand_bits(rng, (1 << L8, B), 0.5)
            base[:, 77] = True
            sizes = ((100003, 0), (90000, 3), (85007, 9), (75000, 2500))
            g = self.ka.Group(self.ctx, K, 1, L8, sum((nf + 127) // 128 * 128 for nf, _ in sizes))
            files = []
            for nf, shift in sizes:                       # column j a copy of base column (7 j + shift) % B
                cmap = (np.arange(nf, dtype=np.int64) * 7 + shift) % B
                files.append((g.add_columns(pack_columns(base[:, cmap], rng), nf), pack_columns(base, rng), nf, cmap))
            g.finalize()
            self.shallow_group = (g, files, L8)
        return self.shallow_group


class Big:
    """One 6 GiB group with its known filters, batches and (lazily) the expected counts of its batch."""

    def __init__(self, env, key):
        ka, oracle = env.ka, env.oracle
        self.key = key
        self.L, self.stride, self.nh, self.reps = GROUPS[key]
        self.nrows = 1 << self.L
        cap = self.stride * 8
        rng = np.random.default_rng(1000 + self.L)
        self.g = g = ka.Group(env.ctx, K, self.nh, self.L, cap)
        assert g.row_stride == self.stride and g.device_bytes == self.nrows * self.stride == 6 * GIB
        assert g.add_random_columns(cap - HEADROOM, 77 + self.L, 64) == 0
        g.finalize()
        fb = self.nrows // 8
        self.filters = np.stack([oracle.bloom_bits_from_sequences([s], K, self.nh, self.L) for s in env.genomes]
                                + [np.full(fb, 255, dtype=np.uint8), np.zeros(fb, dtype=np.uint8)]
                                + [rng.integers(0, 256, size=fb, dtype=np.uint8) for _ in range(2)])
        self.first = g.insert_filters(self.filters)
        assert self.first == cap - HEADROOM and g.column_span == self.first + 8 and g.num_columns == self.first + 7
        self.known = self.first + np.arange(7)
        self.retired = False
        self.base_queries = env.queries
        self.queries = env.queries * self.reps
        self.batch = ka.Batch(env.ctx, self.queries)
        self.batch12 = ka.Batch(env.ctx, env.queries) if self.reps > 1 else self.batch
        self.env, self._exp = env, None
        rng = np.random.default_rng(2000 + self.L)
        self.sample = np.array(sorted(set(ls.rows_around(self.nrows, self.stride)) | set(rng.choice(self.nrows, size=4096, replace=False).tolist())))

    def close(self):
        self.batch.close()
        if self.batch12 is not self.batch:
            self.batch12.close()
        self.g.close()

    def known_filters(self):
        f = self.filters.copy()
        if self.retired:
            f[RETIRED] = 0
        return f

    @property
    def span(self):
        return self.g.column_span

    def expected(self, reps=None):
        """(counts [n, span], nk [n], real [span]) of the batch (`reps` copies of the twelve queries), with the premises
        every test of these groups stands on."""
        if self._exp is None:
            self._exp = ls.Expected(self.env.oracle, self.g.read_rows, self.base_queries, K, self.nh, self.L, self.span)
        e = self._exp
        assert self.nrows * self.stride > 2 ** 32
        offs = e.all_rows() * self.stride
        assert (offs >= 2 ** 32).any() and (offs < 2 ** 32).any()
        for q, gi in self.env.from_genome.items():
            assert e.nk[q] > 0 and e.counts[q, self.known[gi]] == e.nk[q], (q, gi)
        assert 2048 < e.nk.max() < 16384 and e.nk[7] == 0 and e.nk[8] == 1 and np.array_equal(e.counts[10], e.counts[1])
        reps = self.reps if reps is None else reps
        return np.tile(e.counts, (reps, 1)), np.tile(e.nk, reps), self.g.real_columns()

    def genome_records(self, nk):
        """(query, column, num_match) every query cut from a genome must report: its genome's known column, every k-mer."""
        n12 = len(self.base_queries)
        return [(q + rep * n12, int(self.known[gi]), int(nk[q])) for rep in range(len(nk) // n12) for q, gi in self.env.from_genome.items()]


@pytest.fixture(params=KEYS)
def big(request, env):
    return env.group(request.param)


def records_of(hits):
    return set(map(tuple, np.asarray(hits).tolist()))


# ------------------------------------------------------------------------------------------------------------------
# 1. four resident groups whose byte offsets pass 2^32
# ------------------------------------------------------------------------------------------------------------------

def check_known_columns(big):
    """The known columns' bits at the sampled rows: the first row, the last, both sides of byte 2^32 and 4096 more."""
    edge = (1 << 32) // big.stride
    assert {0, big.nrows - 1, edge - 1, edge, edge + 1} <= set(big.sample.tolist())
    assert big.g.row_bytes == big.stride - 15
    got = ls.unpack_columns(big.g.read_rows(big.sample), big.first, 8)
    want = ls.filter_bits_at(big.known_filters(), big.sample)
    assert np.array_equal(got[:, :7], want), np.argwhere(got[:, :7] != want)[:5]
    assert not got[:, 7].any()                            # the pad bit behind them
    assert want[big.sample >= edge + 1, 5].any() and not want[:, 5].all()


def test_inserted_columns(env, big):
    check_known_columns(big)
    for c in (0, 5):                                      # a genome and a random filter: the whole column, through column_bits_kernel and the scan
        fs = env.ka.FilterSet.from_columns(big.g, [int(big.known[c])])
        try:
            want = np.flatnonzero(np.unpackbits(big.filters[c], bitorder="little"))
            assert want[-1] * big.stride >= 2 ** 32 and np.array_equal(fs.rows(0), want), c
        finally:
            fs.close()


def test_group_search(env, big):
    ka, oracle = env.ka, env.oracle
    names = {}
    for batch, reps in ([(big.batch, big.reps)] + ([(big.batch12, 1)] if big.reps > 1 else [])):
        counts, nk, real = big.expected(reps)
        for t in (1.0, 0.8, 0.05):
            exp = ls.hit_records(oracle, counts, nk, real, t)
            for flags in (0, ka.SEARCH_EARLY_EXIT):
                r = big.g.search(batch, t, flags)
                what = "%s n=%d t=%g flags=%d %s" % (big.key, batch.n, t, flags, r.search_kernel)
                assert np.array_equal(r.num_query_kmer, nk), what
                assert_hits_equal(r.hits, exp, what)
                assert set(big.genome_records(nk)) <= records_of(r.hits), what
                names[(batch.n, t, flags)] = r.search_kernel
    print("\nsearch_kernel %s: %s" % (big.key, names))


@pytest.mark.parametrize("key", list(FORMS))
def test_persistent_and_early_exit_forms(env, key):
    """The kernels that compute row addresses of their own: forced where the batch is too small for them by default (the
    several-queries-per-wave forms take no segmented row lists, and the batch's long query is segmented by default)."""
    big = env.group(key)
    counts, nk, real = big.expected()
    for family, t, flags, knobs in FORMS[key]:
        run_forced(env, big, family, t, flags, knobs, counts, nk, real)


def run_forced(env, big, family, t, flags, knobs, counts, nk, real, also=""):
    with env.ctx.tuning(**knobs):
        r = big.g.search(big.batch, t, flags)
    what = "%s %s t=%g flags=%d: %s" % (big.key, family, t, flags, r.search_kernel)
    print("\nforced " + what)
    assert r.search_kernel.startswith(family + "<") and also in r.search_kernel, what
    assert np.array_equal(r.num_query_kmer, nk), what
    assert_hits_equal(r.hits, ls.hit_records(env.oracle, counts, nk, real, t), what)
    left = env.ctx.scratch_nonzero()
    assert not any(left.values()), (what, left)


def test_search_topk(env, big):
    counts, nk, real = big.expected()
    names = set()
    for k in (1, 5, 1024):
        for t in (0.0, 0.8):
            exp = ls.topk_records(env.oracle, counts, nk, real, t, k)
            for knobs in ({}, WHOLE):
                with env.ctx.tuning(**knobs):
                    r = big.g.search_topk(big.batch, k, t)
                what = "%s top-%d t=%g %s" % (big.key, k, t, r.search_kernel)
                assert np.array_equal(r.num_query_kmer, nk), what
                assert_hits_equal(r.hits, exp, what)
                if k >= 5:                                # (the all-ones column ties with the genome's; a single k-mer ties with a quarter of the columns)
                    assert {h for h in big.genome_records(nk) if h[2] >= 20} <= records_of(r.hits), what
                names.add(r.search_kernel)
    print("\ntop-k kernel %s: %s" % (big.key, sorted(names)))


def test_search_scores(env, big):
    import torch
    ka = env.ka
    counts, nk, real = big.expected()
    want = ls.score_matrix(counts, nk, real)
    for q, c, m in big.genome_records(nk):
        assert want[q, c] == m
    sentinel, span = -1234567, big.span
    for knobs in ({}, WHOLE):
        with env.ctx.tuning(**knobs):
            s = big.g.search_scores(big.batch)
            # the device form, into a tensor wider than the span: the cells beyond it stay as they were
            out = torch.full((len(nk), span + 12), sentinel, dtype=torch.int32, device="cuda:%d" % env.ctx.device)
            res = ka.search_scores_device(big.g, big.batch, out)
        assert np.array_equal(s.num_query_kmer, nk), s.kernel
        assert np.array_equal(s.scores, want), (s.kernel, np.argwhere(s.scores != want)[:5])
        got = out.cpu().numpy()
        assert (got[:, span:] == sentinel).all(), res.kernel
        assert np.array_equal(got[:, :span].view(np.uint32), want), (res.kernel, np.argwhere(got[:, :span].view(np.uint32) != want)[:5])
        print("\nscores kernel %s: %s / %s" % (big.key, s.kernel, res.kernel))


def test_search_presence(env, big):
    ka = env.ka
    counts, nk, real = big.expected()
    names = set()
    for t in (1.0, 0.8):
        want = ls.presence_bits(env.oracle, counts, nk, real, t)
        for q, c, _ in big.genome_records(nk):
            assert want[q, c]
        for flags, knobs in ((0, {}), (ka.SEARCH_EARLY_EXIT, {}), (0, WHOLE), (ka.SEARCH_EARLY_EXIT, WHOLE)):
            with env.ctx.tuning(**knobs):
                p = big.g.search_presence(big.batch, t, flags)
            what = "%s t=%g flags=%d %s" % (big.key, t, flags, p.kernel)
            got = p.unpack()
            assert got.shape[1] >= big.span and not got[:, big.span:].any(), what
            assert np.array_equal(got[:, :big.span], want), (what, np.argwhere(got[:, :big.span] != want)[:5])
            assert np.array_equal(p.passing, want.sum(axis=1)) and np.array_equal(p.num_query_kmer, nk), what
            names.add(p.kernel)
    print("\npresence kernel %s: %s" % (big.key, sorted(names)))


def check_column_bits(big):
    """kwage_group_column_bits: the score stage over the identity row list -- 2^L rows, 32-plane counters at L = 24."""
    cb = big.g.column_bits()
    real = big.g.real_columns()
    assert cb.shape == (big.span,) and not cb[~real].any() and (~real).sum() == 1 + big.retired
    assert np.array_equal(cb[big.known], ls.popcount(big.known_filters())), (cb[big.known], ls.popcount(big.known_filters()))
    assert cb[big.known[EMPTY]] == 0 and (big.retired or cb[big.known[ONES]] == 1 << big.L)


def test_column_bits(big):
    check_column_bits(big)


def test_filter_search_sparse_filter(env, big):
    """A filter of ~5000 set rows chosen here, among them the first row, the last and both sides of byte 2^32: every
    column's cell is the sum of those rows' bits."""
    rng = np.random.default_rng(3000 + big.L)
    rows = np.array(sorted(set(ls.rows_around(big.nrows, big.stride)) | set(rng.choice(big.nrows, size=5000, replace=False).tolist())), dtype=np.int64)
    edge = (1 << 32) // big.stride
    assert {0, big.nrows - 1, edge - 1, edge + 1} <= set(rows.tolist()) and (rows * big.stride >= 2 ** 32).sum() > 1000
    bits = np.zeros((1, big.nrows // 8), dtype=np.uint8)
    np.bitwise_or.at(bits[0], rows >> 3, (1 << (rows & 7)).astype(np.uint8))
    real = big.g.real_columns()
    want = np.where(real, ls.column_sums(big.g.read_rows, rows, big.span), 0)
    known_want = ls.filter_bits_at(big.known_filters(), rows).sum(axis=0)
    assert np.array_equal(want[big.known], known_want)          # (read_rows and the known filters agree on these rows)
    fs = env.ka.FilterSet.from_bits(env.ctx, K, big.nh, big.L, bits)
    try:
        assert np.array_equal(fs.rows(0), rows) and fs.bit_counts().tolist() == [rows.size]
        res = big.g.search_filter_scores(fs)
        assert np.array_equal(res.scores[0], want), np.flatnonzero(res.scores[0] != want)[:5]
        print("\nfilter kernel %s (sparse): %s" % (big.key, res.kernel))
    finally:
        fs.close()


def test_filter_search_dense_filters(env, big):
    """The two random known filters as the questions: 2^(L-1) rows each.  The cells of the known columns are the host
    popcounts of the ANDs (the background columns are covered by the addressed-rows cases)."""
    known = big.known_filters()
    fs = env.ka.FilterSet.from_bits(env.ctx, K, big.nh, big.L, big.filters[5:7])
    try:
        assert np.array_equal(fs.bit_counts(), ls.popcount(big.filters[5:7]))
        res = big.g.search_filter_scores(fs)
        for i in range(2):
            want = ls.popcount(big.filters[5 + i][None, :] & known)
            assert np.array_equal(res.scores[i, big.known], want), (i, res.scores[i, big.known], want)
        assert res.scores[0, big.known[5]] == ls.popcount(big.filters[5]) > (1 << big.L) // 3
        assert not res.scores[:, ~big.g.real_columns()].any()
        print("\nfilter kernel %s (dense): %s" % (big.key, res.kernel))
    finally:
        fs.close()


def test_retire_a_known_column(env, big):
    """The all-ones column -- until now reported by every query with k-mers -- becomes a pad column.  (Last of the tests
    of these groups: the module's groups are shared.  With the densest column gone the truncated count walk can plan a
    cut, so that form runs here.)"""
    ka, oracle = env.ka, env.oracle
    col = int(big.known[RETIRED])
    if not big.retired:
        counts, nk, real = big.expected()
        assert real[col] and (counts[nk > 0, col] == nk[nk > 0]).all()
        before = big.g.num_columns
        big.g.retire_columns([col])
        big.retired, big._exp = True, None
        assert big.g.num_columns == before - 1
    counts, nk, real = big.expected()                     # from the rows as they are now
    assert not real[col] and not counts[:, col].any()
    check_known_columns(big)                              # zero where it was, its neighbours unchanged
    check_column_bits(big)
    for t in (1.0, 0.8):
        exp = ls.hit_records(oracle, counts, nk, real, t)
        assert col not in exp["column"] and exp.size
        for flags in (0, ka.SEARCH_EARLY_EXIT):
            assert_hits_equal(big.g.search(big.batch, t, flags).hits, exp, "%s retired t=%g flags=%d" % (big.key, t, flags))
        p = big.g.search_presence(big.batch, t)
        assert np.array_equal(p.unpack()[:, :big.span], ls.presence_bits(oracle, counts, nk, real, t))
    r = big.g.search_topk(big.batch, 5)
    assert_hits_equal(r.hits, ls.topk_records(oracle, counts, nk, real, 0.0, 5), big.key + " retired top-5")
    assert col not in r.hits["column"]
    assert np.array_equal(big.g.search_scores(big.batch).scores, ls.score_matrix(counts, nk, real))
    fs = ka.FilterSet.from_bits(env.ctx, K, big.nh, big.L, big.filters[5:6])
    try:
        got = big.g.search_filter_scores(fs).scores[0]
        assert got[col] == 0 and np.array_equal(got[big.known], ls.popcount(big.filters[5][None, :] & big.known_filters()))
    finally:
        fs.close()
    if big.stride >= 1024:
        run_forced(env, big, "count_walk_kernel", 0.8, EE, ss.TRUNC, counts, nk, real, also=",trunc>+refine<")


# ------------------------------------------------------------------------------------------------------------------
# 2. results that pass 2^32 bytes
# ------------------------------------------------------------------------------------------------------------------

def compare_cyclic(out, exp8):
    """out [n, w] on the device, row i expected to be exp8[i % 8]: compared there, 64 groups of eight rows at a time.
    Returns the first differing row, or None."""
    import torch
    v = out.view(-1, 8, out.shape[1])
    ok = torch.ones((), dtype=torch.bool, device=out.device)
    for a in range(0, v.shape[0], 64):
        ok &= (v[a:a + 64] == exp8[None]).all()
    if bool(ok):
        return None
    for a in range(v.shape[0]):
        same = (v[a] == exp8).all(dim=1)
        if not bool(same.all()):
            return 8 * a + int(torch.nonzero(~same)[0])
    raise AssertionError("unreachable")


def shallow_counts(env, pool):
    g, files, L8 = env.shallow()
    span = g.column_span
    counts = np.zeros((len(pool), span), dtype=np.int64)
    nk = np.zeros(len(pool), dtype=np.uint32)
    for q, seq in enumerate(pool):
        kmers = env.oracle.unique_kmers(seq, K)
        nk[q] = len(kmers)
        if len(kmers):
            counts[q] = np.maximum(column_counts(env.oracle, files, span, K, 1, L8, kmers), 0)
    return counts, nk


def test_scores_written_beyond_byte_2_to_the_32(env):
    import torch
    ka = env.ka
    g, files, L8 = env.shallow()
    rng = np.random.default_rng(42)
    pool = [ls.random_dna(rng, 150), ls.random_dna(rng, 60), "ACGT", ls.random_dna(rng, 400), ls.random_dna(rng, K), ls.random_dna(rng, 90),
            ls.random_dna(rng, 33), ls.random_dna(rng, 200)]
    counts, nk = shallow_counts(env, pool)
    span, sentinel = g.column_span, -1234567
    row_elems = span + 4
    n = (-(-2 ** 32 // (row_elems * 4)) + 1 + 7) // 8 * 8
    assert n * row_elems * 4 > 2 ** 32 and (n - 1) * row_elems * 4 >= 2 ** 32        # the last query's row lies wholly beyond byte 2^32
    exp8 = np.full((8, row_elems), sentinel, dtype=np.int32)
    exp8[:, :span] = ls.score_matrix(counts, nk, g.real_columns()).view(np.int32)
    assert exp8[0, :span].max() == nk[0] == 120 and not exp8[2, :span].any() and len({r.tobytes() for r in exp8}) == 8
    dev = torch.device("cuda", env.ctx.device)
    b = ka.Batch(env.ctx, [pool[i % 8] for i in range(n)])
    out = torch.full((n, row_elems), sentinel, dtype=torch.int32, device=dev)
    try:
        t0 = time.perf_counter()
        res = ka.search_scores_device(g, b, out)
        bad = compare_cyclic(out, torch.from_numpy(exp8).to(dev))            # every row, the last one among them
        print("\nscores beyond 2^32: n=%d, %.2f GB, %s, search + compare %.2f s" % (n, n * row_elems * 4 / 1e9, res.kernel, time.perf_counter() - t0))
        assert bad is None, (bad, bad * row_elems * 4)
    finally:
        b.close()
        del out
        torch.cuda.empty_cache()


def test_presence_written_beyond_byte_2_to_the_32(env):
    import torch
    from kwage_amd.engine import presence_row_bytes
    ka, oracle = env.ka, env.oracle
    g, files, L8 = env.shallow()
    rng = np.random.default_rng(43)
    pool = [ls.random_dna(rng, K + 4) for _ in range(6)] + ["ACGTACGT", ls.random_dna(rng, K + 1)]      # a few k-mers each: a short gather
    counts, nk = shallow_counts(env, pool)
    t, W = 0.8, presence_row_bytes(g)
    n = (-(-2 ** 32 // W) + 1 + 7) // 8 * 8
    assert n * W > 2 ** 32 and (n - 1) * W >= 2 ** 32
    want = ls.presence_bits(oracle, counts, nk, g.real_columns(), t)
    exp8 = np.zeros((8, W), dtype=np.uint8)
    exp8[:, :g.row_bytes] = np.packbits(want, axis=1, bitorder="little")
    assert nk.tolist() == [5] * 6 + [0, 2] and all(0 < r.sum() < g.num_columns for r in want[:6]) and not want[6].any()
    dev = torch.device("cuda", env.ctx.device)
    b = ka.Batch(env.ctx, [pool[i % 8] for i in range(n)])
    out = torch.full((n, W), 0xA5, dtype=torch.uint8, device=dev)
    try:
        t0 = time.perf_counter()
        res = ka.search_presence_device(g, b, t, out)
        bad = compare_cyclic(out, torch.from_numpy(exp8).to(dev))
        print("\npresence beyond 2^32: n=%d, %.2f GB, %s, search + compare %.2f s" % (n, n * W / 1e9, res.kernel, time.perf_counter() - t0))
        assert bad is None, (bad, bad * W)
    finally:
        b.close()
        del out
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# 3. the insert's staged chunks
# ------------------------------------------------------------------------------------------------------------------

L20 = 20
FILTER_BYTES = (1 << L20) // 8
STAGING = 64 << 20            # insert.hip insert_from_host: a call's filters above this are staged in chunks of rows
FILTERS_PER_TILE = 1024       # insert.hip InsertTile: one launch of the device form covers more than one tile beyond this


@pytest.fixture(scope="module")
def pool20():
    """1100 filters of 2^20 bits at density 1/2 and the five that go in first (shared, never changed)."""
    rng = np.random.default_rng(20)
    return rng.integers(0, 256, size=(5, FILTER_BYTES), dtype=np.uint8), rng.integers(0, 256, size=(1100, FILTER_BYTES), dtype=np.uint8)


def chunk_rows_of(n):
    """insert_from_host's rule restated: halve the chunk until its n pieces fit the staging."""
    rows = 1 << L20
    while rows > 1024 and rows // 8 * n > STAGING:
        rows //= 2
    return rows


def sample_rows20(n):
    rng = np.random.default_rng(21)
    step = chunk_rows_of(n)
    edges = {r for b in range(step, 1 << L20, step) for r in (b - 1, b)}
    return np.array(sorted({0, 1, (1 << L20) - 1} | edges | set(rng.choice(1 << L20, size=4096, replace=False).tolist())))


def check_staged(env, five, filters, g, rows):
    """What every form must leave behind: the bits of the host filters at the sampled rows (the five earlier columns
    included), zero up to the stride, and after finalize every column's set bits and four whole columns."""
    ka, n = env.ka, filters.shape[0]
    everything = np.concatenate([five, filters])
    assert g.row_bytes == (5 + n + 7) // 8 and g.num_columns == 5 + n
    got = g.read_rows(rows)
    want = ls.filter_bits_at(everything, rows)
    cols = ls.unpack_columns(got, 0, 8 * g.row_bytes)
    assert np.array_equal(cols[:, :5 + n], want), np.argwhere(cols[:, :5 + n] != want)[:5]
    assert not cols[:, 5 + n:].any()
    # the rest of the row: one-column blocks on every further 16-byte boundary make it visible (test_gpu_live_insert.py)
    one = np.zeros((1 << L20, 1), dtype=np.uint8)
    blocks = 0
    while (g.row_bytes + 15) // 16 * 16 < g.row_stride:
        g.add_columns(one, 1)
        blocks += 1
    rest = g.read_rows(rows)
    assert blocks >= 1 and np.array_equal(rest[:, :got.shape[1]], got) and not rest[:, got.shape[1]:].any()
    g.finalize()
    assert np.array_equal(g.column_bits()[:5 + n], ls.popcount(everything))
    for i in (0, n // 3, 2 * n // 3, n - 1):
        fs = ka.FilterSet.from_columns(g, [5 + i])
        try:
            assert np.array_equal(fs.rows(0), np.flatnonzero(np.unpackbits(filters[i], bitorder="little"))), i
        finally:
            fs.close()
    return got


@pytest.mark.parametrize("form,n,chunks", [("packed", 520, 2), ("packed", 1100, 4), ("strided", 520, 2), ("strided", 1100, 4),
                                           ("bloom files", 520, 2), ("device", 1100, 4)])
def test_insert_of_more_than_the_staging_holds(env, oracle, pool20, tmp_path, form, n, chunks):
    import torch
    ka = env.ka
    five, filters = pool20[0], pool20[1][:n]
    assert n * (2 ** L20 // 8) > 64 << 20                  # insert.hip insert_from_host: above 64 MiB the filters are staged in chunks of rows
    assert (1 << L20) // chunk_rows_of(n) == chunks and chunk_rows_of(8) == 1 << L20
    rows = sample_rows20(n)
    assert {chunk_rows_of(n) - 1, chunk_rows_of(n), (chunks - 1) * chunk_rows_of(n)} <= set(rows.tolist())
    g = ka.Group(env.ctx, K, 2, L20, 2048)
    twin = None
    try:
        assert g.insert_filters(five) == 0                # the bit offset of what follows is no multiple of 32
        if form == "packed":
            assert filters.strides[0] == FILTER_BYTES
            first = g.insert_filters(filters)
        elif form == "strided":                           # filters 24 bytes further apart than they are long: the pitched copy
            wide = np.random.default_rng(22).integers(0, 256, size=(n, FILTER_BYTES + 24), dtype=np.uint8)
            wide[:, :FILTER_BYTES] = filters
            first = g.insert_filters(wide)
        elif form == "bloom files":
            paths = []
            for i in range(n):
                paths.append(str(tmp_path / ("s%04d.bloom" % i)))
                oracle.write_bloom(paths[-1], K, L20, 2, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (7000 + i))), filters[i])
            first = g.insert_bloom_files(paths)
        else:                                             # the device form stages nothing, but its one launch covers two tiles of filters
            assert n > FILTERS_PER_TILE
            first = g.insert_filters(torch.from_numpy(filters).to(torch.device("cuda", env.ctx.device)))
        assert first == 5
        got = check_staged(env, five, filters, g, rows)
        if form == "packed":                              # eight at a time never chunks: the same rows
            twin = ka.Group(env.ctx, K, 2, L20, 2048)
            assert twin.insert_filters(five) == 0
            for i in range(0, n, 8):
                assert twin.insert_filters(filters[i:i + 8]) == 5 + i
            assert np.array_equal(twin.read_rows(rows), got)
    finally:
        g.close()
        if twin is not None:
            twin.close()
