"""The k-mer stage (kmer_kernel + kmer_finish_kernel) in every launch form of tests/kmer_shapes.py, through kwage_hash_batch
and kwage_search, bit for bit against the oracle (unique_kmers / row_indices / query_threshold, themselves pinned to the
reference binary's KATs).  tests/test_kmer_shapes_ledger.py checks on CPU that the batches reach every form.

The device's k-mers of a query are sorted and its rows permuted alike, so each k-mer stays paired with its own rows; every
query of every batch is compared, so a write outside a query's own [pos_off[q], pos_off[q+1]) shows up in its neighbour.

(a) + (b) test_every_form: each batch of the table at k = 1, 4, 15, 31, 32 with the adversarial queries built for its
    workgroup size; num_hash 1...5 and L = 0, 1, 20, 31, 32.
(c) test_query_threshold_at_both_code_sites: the float32 floor written by thread 0 and by kmer_finish_kernel.
(d) test_state_carried_between_launches: one batch at two k, long tables before short ones, repeated launches, no queries.
(e) test_many_reads: 20 000 reads, one 64-thread workgroup each."""
import ctypes as C

import numpy as np
import pytest

import kmer_shapes as ks

pytestmark = pytest.mark.gpu

KS = (1, 4, 15, 31, 32)
MAX_HASH = 5
INVALID = "Nnx"                       # an invalid base: N, a lower-case n, any other byte
_RC = str.maketrans("ACGT", "TGCA")


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


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def revcomp(s):
    return s.translate(_RC)[::-1]


def positions(seq, k):
    return max(len(seq) - k + 1, 0)


# ---- the queries of a batch ----------------------------------------------------------------------------------------------
def adversarial(rng, P, k, T):
    """(b): the queries built for a launch of T threads, each of at most P positions (n = P + k - 1 characters)."""
    n, Cq = P + k - 1, ks.KM_CHUNK
    out = []
    # one invalid base: first and last character, then in and just past the k - 1 characters two tiles / two chunks both stage
    offsets = [0, n - 1, T - 1, T, T + k - 2, T + k - 1, 2 * T - 1, Cq - 1, Cq, Cq + k - 2, Cq + k - 1]
    for i, off in enumerate(dict.fromkeys(offsets)):
        if 0 <= off < n:
            s = rand_seq(rng, n)
            # the kind rotates with k as well: over the five k every offset sees an N, an n and an x
            out.append(s[:off] + INVALID[(i + k) % 3] + s[off + 1:])
    half = rand_seq(rng, (n + 1) // 2)
    out.append((half + revcomp(half))[:n])           # the same canonical words again in later tiles and chunks
    out.append("A" * n)                              # one k-mer: every lane on one slot of the set
    out.append(("AT" * n)[:n])                       # one or two
    out.append(("ACGTTCA" * (n // 7 + 1))[:n])       # a period-7 repeat
    if k in (4, 32):                                 # words equal to their own reverse complement
        words = [h + revcomp(h) for h in (rand_seq(rng, k // 2) for _ in range(n // k + 1))]
        out.append("".join(words)[:n])
    return out


def batch_queries(P, k):
    """The batch of the table whose longest query has P positions, at k-mer length k: the boundary query first."""
    rng = np.random.default_rng(1000 * P + k)
    n = P + k - 1
    half = rand_seq(rng, P // 2 + k - 1)
    # "N"*60 is cut to the boundary query's length: at k = 1 sixty Ns have 60 positions, which would make them the longest
    # query of every batch below P = 60 and move that batch to another form
    seqs = [rand_seq(rng, n), "", rand_seq(rng, k - 1), rand_seq(rng, k), "N" * min(60, n), half, half.lower()]
    seqs += adversarial(rng, P, k, ks.threads(P))
    assert positions(seqs[0], k) == P == max(positions(s, k) for s in seqs)      # the launch is sized by the boundary query
    return seqs


# ---- device and oracle ---------------------------------------------------------------------------------------------------
def hash_once(ctx, batch, seqs, k, nh, L):
    """ONE launch of the stage (kwage_hash_batch) -> per query (sorted k-mers, their rows [n, nh])."""
    from kwage_amd import native
    n = len(seqs)
    exp_offs = np.zeros(n + 1, dtype=np.uint64)
    exp_offs[1:] = np.cumsum([positions(s, k) for s in seqs], dtype=np.uint64)
    total = int(exp_offs[-1])
    offs, nk = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
    kmers, rows = np.zeros(max(total, 1), dtype=np.uint64), np.zeros(max(total, 1) * nh, dtype=np.uint32)
    p = native.Params(k, nh, L, 0)
    native.check(native.lib().kwage_hash_batch(ctx._h, C.byref(p), batch._h, offs.ctypes.data, nk.ctypes.data,
                                               kmers.ctypes.data, rows.ctypes.data))
    assert np.array_equal(offs, exp_offs)
    over = np.flatnonzero(nk[:n] > np.diff(exp_offs))
    assert over.size == 0, ("more k-mers than positions", over[:5].tolist(), nk[over[:5]].tolist())
    rows = rows.reshape(-1, nh)
    out = []
    for q in range(n):
        o, m = int(offs[q]), int(nk[q])
        order = np.argsort(kmers[o:o + m], kind="stable")
        out.append((kmers[o:o + m][order], rows[o:o + m][order]))
    return out


def expected(oracle, seqs, k):
    """Per query (sorted distinct canonical k-mers, the five unmasked hashes of each): hash h does not depend on num_hash."""
    kmers = [oracle.unique_kmers(s, k) for s in seqs]
    return kmers, [oracle.row_indices(km, k, MAX_HASH, 32) for km in kmers]


def assert_stage(got, exp, nh, L, what):
    kmers, hashes = exp
    mask = np.uint32(0xFFFFFFFF if L >= 32 else (1 << L) - 1)
    assert len(got) == len(kmers)
    for q, (km, rw) in enumerate(got):
        assert np.array_equal(km, kmers[q]), (what, "nh", nh, "L", L, "query", q, "device", len(km), "oracle", len(kmers[q]))
        assert np.array_equal(rw, hashes[q][:, :nh] & mask), (what, "nh", nh, "L", L, "query", q, "rows")


def assert_same(a, b, what):
    assert len(a) == len(b)
    for q, ((ka_, ra), (kb, rb)) in enumerate(zip(a, b)):
        assert np.array_equal(ka_, kb) and np.array_equal(ra, rb), (what, "query", q)


# ---- (a) + (b) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("batch", ks.BATCHES, ids=lambda b: "P%d" % b.max_pos)
def test_every_form(ka, ctx, oracle, batch, k):
    """Nothing here observes the form the device launched: that this batch lands in batch.form rests on the CPU ledger
    (tests/test_kmer_shapes_ledger.py), which holds the table's constants to the sources.  The assertion below only keeps
    the table consistent with its own rules."""
    P = batch.max_pos
    assert batch.form == ks.form(P)
    seqs = batch_queries(P, k)
    exp = expected(oracle, seqs, k)
    if k == 31:                        # half + its reverse complement: every word of the second half is one of the first
        assert positions(seqs[-4], k) == P and len(exp[0][-4]) <= (P + 1) // 2
    b = ka.Batch(ctx, seqs)
    try:
        for nh in range(1, MAX_HASH + 1):
            assert_stage(hash_once(ctx, b, seqs, k, nh, 20), exp, nh, 20, ("P", P, "k", k))
        for L in (0, 1, 31, 32):
            assert_stage(hash_once(ctx, b, seqs, k, 3, L), exp, 3, L, ("P", P, "k", k))
    finally:
        b.close()


# ---- (c) -----------------------------------------------------------------------------------------------------------------
THRESHOLDS = [np.float32(t) for t in (1e-7, 0.05, 0.1, 0.3, 0.5, 0.7, 0.9, 0.95, 0.99)] + [np.nextafter(np.float32(1), np.float32(0))]
DISTINCT = (1, 10, 100, 5000)
# (t, n) at which a float32 product and a double product of float32(t) and n truncate differently
F32_ONLY = ((0.7, 10), (0.7, 100), (0.7, 5000), (0.9, 10), (0.9, 100), (0.9, 5000), (0.95, 100), (0.95, 5000))


def query_with(oracle, n, k=31):
    """A random query of exactly n distinct k-mers (n + k - 1 bases; drawn again from the next seed if two coincide)."""
    seed = 7000 + n
    while True:
        s = rand_seq(np.random.default_rng(seed), n + k - 1)
        if len(oracle.unique_kmers(s, k)) == n:
            return s
        seed += 1


def test_query_threshold_at_both_code_sites(ka, ctx, oracle):
    k = 31
    ns = sorted(set(DISTINCT) | set(ks.MAX_POS))
    # the grid separates float32 from double: an implementation whose product is a double cannot pass
    f32 = {(t, n): int(np.float32(t) * np.float32(n)) for t in THRESHOLDS for n in ns}
    f64 = {(t, n): int(float(t) * n) for t in THRESHOLDS for n in ns}
    for (t, n), v in f32.items():
        assert oracle.query_threshold(float(t), n) == v, (t, n)
    differ = {(float(t), n) for (t, n) in f32 if f32[t, n] != f64[t, n]}
    assert {(float(np.float32(t)), n) for t, n in F32_ONLY} <= differ, differ
    assert (f32[np.float32(0.7), 10], f64[np.float32(0.7), 10]) == (7, 6) and (f32[np.float32(0.95), 5000], f64[np.float32(0.95), 5000]) == (4750, 4749)
    assert THRESHOLDS[-1] < 1 and f32[THRESHOLDS[-1], 5000] == 4999

    queries = {n: query_with(oracle, n, k) for n in ns}
    g = ka.Group(ctx, k, 1, 8, 8)
    g.add_columns(np.zeros((1 << 8, 1), dtype=np.uint8), 8)
    g.finalize()
    try:
        # longest query 100: every value written by thread 0 of a 64-thread workgroup; 2048: by thread 0 of 256; 5000: a
        # multi-chunk query in the batch, every value -- the short queries' too -- rewritten by kmer_finish_kernel
        for longest in (100, ks.MULTI_EDGE, 5000):
            sizes = [n for n in ns if n <= longest]
            assert ks.form(max(sizes)).finish == (longest == 5000)
            seqs = [queries[n] for n in sizes] + ["", "ACGT"]
            b = ka.Batch(ctx, seqs)
            try:
                for t in THRESHOLDS:
                    r = g.search(b, float(t))
                    exp_n = sizes + [0, 0]
                    assert r.num_query_kmer.tolist() == exp_n, (longest, t)
                    exp_t = [oracle.query_threshold(float(t), n) for n in exp_n]
                    assert r.query_threshold.tolist() == exp_t, (longest, float(t), [(n, got, e) for n, got, e in
                                                                                      zip(exp_n, r.query_threshold.tolist(), exp_t) if got != e])
            finally:
                b.close()
    finally:
        g.close()


# ---- (d) -----------------------------------------------------------------------------------------------------------------
def test_state_carried_between_launches(ka, oracle):
    nh, L = 3, 20
    with ka.Context(0) as ctx:
        # no queries at all, then queries without a position
        for seqs in ([], ["", "ACG"]):
            b = ka.Batch(ctx, seqs)
            got = hash_once(ctx, b, seqs, 31, nh, L)
            b.close()
            assert [len(km) for km, _ in got] == [0] * len(seqs)

        long_a, short, long_b = batch_queries(5000, 31), batch_queries(2049, 31), batch_queries(5000, 15)
        # one Batch at k = 31, 15, 31: the layout of each k is built once and kept with the batch.  As many queries as the long
        # batches below, so that every per-query count those accumulate into holds a stale non-zero value from here on
        rng = np.random.default_rng(77)
        seqs = batch_queries(768, 31)
        seqs += [rand_seq(rng, 100) for _ in range(max(len(long_a), len(long_b)) - len(seqs))]
        exp = {k: expected(oracle, seqs, k) for k in (31, 15)}
        b = ka.Batch(ctx, seqs)
        try:
            for k in (31, 15, 31, 15):
                got = hash_once(ctx, b, seqs, k, nh, L)
                assert_stage(got, exp[k], nh, L, ("one batch at k", k))
                fresh = ka.Batch(ctx, seqs)
                try:
                    assert_same(got, hash_once(ctx, fresh, seqs, k, nh, L), ("fresh batch at k", k))
                finally:
                    fresh.close()
        finally:
            b.close()

        # long global tables, then shorter ones at the same place, then the long ones again: tables cleared, counts zeroed
        for seqs, k in ((long_a, 31), (short, 31), (long_a, 31), (long_b, 15), (short, 31)):
            exp_k = expected(oracle, seqs, k)
            b = ka.Batch(ctx, seqs)
            try:
                first = hash_once(ctx, b, seqs, k, nh, L)
                assert_stage(first, exp_k, nh, L, ("positions", positions(seqs[0], k), "k", k))
                assert_same(first, hash_once(ctx, b, seqs, k, nh, L), "second launch of the same batch")
            finally:
                b.close()


# ---- (e) -----------------------------------------------------------------------------------------------------------------
def test_many_reads(ka, ctx, oracle):
    k, nh, L, n_reads = 31, 3, 20, 20000
    rng = np.random.default_rng(20000)
    genome = rand_seq(rng, 400000)
    starts, lengths = rng.integers(0, len(genome) - 150, size=n_reads), rng.integers(100, 151, size=n_reads)
    reads = [genome[s:s + n] for s, n in zip(starts.tolist(), lengths.tolist())]
    for i in range(0, n_reads, 11):                   # some with an invalid base, some lower-case, some reverse strands
        off = int(rng.integers(0, len(reads[i])))
        reads[i] = reads[i][:off] + INVALID[i % 3] + reads[i][off + 1:]
    for i in range(5, n_reads, 13):
        reads[i] = revcomp(reads[i]).lower()
    assert ks.form(max(positions(r, k) for r in reads)) == ks.Form(64, 256, 1, False)
    b = ka.Batch(ctx, reads)
    try:
        got = hash_once(ctx, b, reads, k, nh, L)
    finally:
        b.close()
    mask = np.uint32((1 << L) - 1)
    for i, (r, (km, rw)) in enumerate(zip(reads, got)):
        exp = oracle.unique_kmers(r, k)
        assert np.array_equal(km, exp), (i, len(km), len(exp))
        if i % 97 == 0:
            assert np.array_equal(rw, oracle.row_indices(exp, k, nh, 32) & mask), i
