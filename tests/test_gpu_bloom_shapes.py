"""Database construction from sequences in every case of tests/bloom_shapes.py -- the shared-set launch form of kmer_kernel
through kwage_bloom_bits_from_batch / kwage_count_distinct_kmers ("B") and behind the piece cut of kwage_make_bloom ("M")
-- bit for bit against the oracle (bloom_bits_from_sequences / unique_kmers / write_bloom, themselves pinned to files the
reference wrote).  tests/test_bloom_shapes_ledger.py checks on CPU that the table is what it says and that no case's filter
is saturated.  One context for the module; every comparison is exact.

(a) test_every_case: filter, distinct count, `.bloom` file, and the bytes behind the caller's buffer.
(b) test_filter_of_2_pow_32_bits: the one large case, compared by its set bits.
(c) test_state_between_constructions / test_search_construction_search: what one call leaves for the next on slot 0.
(d) test_no_false_negative_through_the_chain: make_bloom -> build_db -> add_db_file -> search at t = 1."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import bloom_shapes as bs

pytestmark = pytest.mark.gpu

GUARD = 64                             # bytes behind the caller's buffer
ACCESSION = "SRR424242"


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


# ---- device and oracle ---------------------------------------------------------------------------------------------------
def sample_info(oracle):
    """The same record on both sides: (kwage_sample_info, what it points to), oracle.FilterInfo."""
    from kwage_amd import native
    tags, vals = (C.c_char_p * 1)(b"isolate"), (C.c_char_p * 1)(b"shape table")
    si = native.SampleInfo()
    si.run_accession, si.experiment_title, si.sample_taxa = ACCESSION.encode(), b"construction cases", b"synthetic construct"
    si.attribute_tags, si.attribute_values, si.num_attributes = tags, vals, 1
    si.number_of_spots, si.number_of_bases = 7, 1234
    si.day, si.month, si.year = 3, 2, 2021
    fi = oracle.FilterInfo(run_accession=oracle.str_to_accession(ACCESSION), experiment_title="construction cases", sample_taxa="synthetic construct",
                           sample_attributes=[("isolate", "shape table")], number_of_spots=7, number_of_bases=1234, date=(3, 2, 2021))
    return si, (tags, vals), fi


def device_bits(ka, ctx, seqs, k, nh, L):
    """B: (filter bytes, distinct of kwage_bloom_bits_from_batch, distinct of kwage_count_distinct_kmers); the guard is checked."""
    from kwage_amd import native
    nbytes = ((1 << L) + 7) // 8
    buf = np.full(nbytes + GUARD, 0xA5, dtype=np.uint8)
    prm, nd, cnt = native.Params(k, nh, L, 0), C.c_uint64(1 << 60), C.c_uint64(1 << 60)
    b = ka.Batch(ctx, seqs)
    try:
        native.check(native.lib().kwage_bloom_bits_from_batch(ctx._h, C.byref(prm), b._h, buf.ctypes.data, C.byref(nd)))
        native.check(native.lib().kwage_count_distinct_kmers(ctx._h, b._h, k, C.byref(cnt)))
    finally:
        b.close()
    assert np.all(buf[nbytes:] == 0xA5), "bytes behind ceil(2^L / 8) of the caller's buffer were written"
    return buf[:nbytes], nd.value, cnt.value


def device_file(ctx, oracle, seqs, k, nh, L, path):
    """M: kwage_make_bloom of the sequences into `path` -> its distinct count."""
    from kwage_amd import native
    raw = [s.encode("latin-1") for s in seqs]
    offs = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        offs[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
    si, keep, _ = sample_info(oracle)
    prm, nd = native.Params(k, nh, L, 0), C.c_uint64(1 << 60)
    native.check(native.lib().kwage_make_bloom(ctx._h, C.byref(prm), b"".join(raw), offs.ctypes.data, len(raw), C.byref(si), str(path).encode(), C.byref(nd)))
    return nd.value


def oracle_bits(oracle, case):
    return oracle.bloom_bits_from_sequences(bs.distinct_seqs(case.seqs), case.k, case.num_hash, case.L)


def run_case(ka, ctx, oracle, case, tmp_path, want_bits=None):
    """Every entry point of the case against the oracle; returns what the device gave, for the state tests to compare."""
    want_bits = oracle_bits(oracle, case) if want_bits is None else want_bits
    want_distinct = len(bs.expected(oracle, case)[0])
    got = {}
    if "B" in case.entry:
        bits, nd, cnt = device_bits(ka, ctx, case.seqs, case.k, case.num_hash, case.L)
        assert (nd, cnt) == (want_distinct, want_distinct), (case.name, "distinct", nd, cnt, "oracle", want_distinct)
        assert np.array_equal(bits, want_bits), (case.name, "B", "bits set: device", int(np.unpackbits(bits).sum()), "oracle", int(np.unpackbits(want_bits).sum()))
        got["B"] = (bits.tobytes(), nd, cnt)
    if "M" in case.entry:
        out, ref = tmp_path / (case.name + ".bloom"), tmp_path / (case.name + ".oracle.bloom")
        nd = device_file(ctx, oracle, case.seqs, case.k, case.num_hash, case.L, out)
        assert nd == want_distinct, (case.name, "M", "distinct", nd, "oracle", want_distinct)
        prm, _, _, file_bits = oracle.read_bloom(str(out))
        assert prm == (case.k, case.L, case.num_hash, 0), case.name
        assert np.array_equal(file_bits, want_bits), (case.name, "M", "bits set: device", int(np.unpackbits(file_bits).sum()), "oracle", int(np.unpackbits(want_bits).sum()))
        oracle.write_bloom(str(ref), case.k, case.L, case.num_hash, sample_info(oracle)[2], want_bits)
        data = out.read_bytes()
        assert data == ref.read_bytes(), (case.name, "the .bloom file")
        got["M"] = (data, nd)
    if case.empty:
        assert want_distinct == 0 and not want_bits.any(), case.name
    return got


# ---- (a) -----------------------------------------------------------------------------------------------------------------
SMALL = [c for c in bs.CASES if c.L < 32]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_every_case(ka, ctx, oracle, tmp_path, case):
    """Nothing here observes the launch form or the pieces: that kwage_make_bloom cuts these sequences as bloom_shapes.pieces
    does and that the shared set has table_log2 slots rests on the CPU ledger, which holds both to the sources.  The cases
    of the piece cut run the same sequences cut (M) and uncut (B): run_case holds both to one oracle filter."""
    run_case(ka, ctx, oracle, case, tmp_path)


# ---- (b) -----------------------------------------------------------------------------------------------------------------
def test_filter_of_2_pow_32_bits(ka, ctx, oracle, tmp_path):
    """L = 32: row_mask is all ones (its own branch), the filter is 512 MiB.  Compared by the indices of its non-zero bytes and
    those bytes, not element by element."""
    case, = [c for c in bs.CASES if c.L == 32]
    free, _ = ctx.mem_info()
    if free < (2 << 30):
        pytest.skip("not enough free HBM for a 512 MiB filter")
    want = oracle_bits(oracle, case)
    want_at = np.flatnonzero(want)
    want_distinct = len(bs.expected(oracle, case)[0])
    assert 0 < len(want_at) <= want_distinct * case.num_hash and int(np.unpackbits(want[want_at]).sum()) == len(bs.expected(oracle, case)[1])
    bits, nd, cnt = device_bits(ka, ctx, case.seqs, case.k, case.num_hash, case.L)
    at = np.flatnonzero(bits)
    assert (nd, cnt) == (want_distinct, want_distinct)
    assert np.array_equal(at, want_at) and np.array_equal(bits[at], want[want_at])
    del bits
    out = tmp_path / "L32.bloom"
    assert device_file(ctx, oracle, case.seqs, case.k, case.num_hash, case.L, out) == want_distinct
    head = b"\xff" + struct.pack("<IIIiI", case.k, case.L, case.num_hash, 0, zlib.crc32(want) & 0xFFFFFFFF) + oracle.pack_filter_info(sample_info(oracle)[2])
    with open(out, "rb") as f:
        assert f.read(len(head)) == head
    payload = np.memmap(str(out), dtype=np.uint8, mode="r", offset=len(head))
    assert payload.size == 1 << 29
    at = np.flatnonzero(payload)
    assert np.array_equal(at, want_at) and np.array_equal(payload[at], want[want_at])


# ---- (c) -----------------------------------------------------------------------------------------------------------------
def test_state_between_constructions(ka, ctx, oracle, tmp_path):
    """Two cases of different k and L alternately on one context: a long sample's table, counters and filter length must
    leave nothing for a short one, and the other way round."""
    a, b = bs.BY_NAME["cut_k31_sample_pieces5"], bs.BY_NAME["len_L8_h1_sample"]
    assert (a.k, a.L) != (b.k, b.L) and bs.table_log2(bs.total_pos(a.seqs, a.k)) > bs.table_log2(bs.total_pos(b.seqs, b.k))
    want = {c.name: oracle_bits(oracle, c) for c in (a, b)}
    first = {}
    for rep in range(3):
        for c in (a, b):
            d = tmp_path / ("rep%d" % rep)
            d.mkdir(exist_ok=True)
            got = run_case(ka, ctx, oracle, c, d, want[c.name])
            assert first.setdefault(c.name, got) == got, (c.name, "repetition", rep)


def test_search_construction_search(ka, ctx, oracle, tmp_path):
    """The construction borrows slot 0's tables, counters and result layout from the search: a threshold search before it,
    after a short sample and after a long one reports the same hit list.  The batch has a query long enough for the
    global-table form of the search's own k-mer stage (more than 2048 positions)."""
    k, nh, L, ncol = 31, 3, 12, 40
    rng = np.random.default_rng(4242)
    rows = np.packbits(rng.random((1 << L, ncol)) < 0.5, axis=1, bitorder="little")
    queries = [bs.rand_seq(rng, n) for n in (100, 31, 30, 3000, 150, 0, 600)] + ["N" * 50]
    g = ka.Group(ctx, k, nh, L, ncol)
    g.add_columns(rows, ncol)
    g.finalize()
    b = ka.Batch(ctx, queries)
    try:
        def search():
            r = g.search(b, 0.1)
            return r.hits.tobytes(), r.num_query_kmer.tolist(), r.query_threshold.tolist()
        before = search()
        assert len(before[0]) > 0 and before[1] == [len(oracle.unique_kmers(q, k)) for q in queries]
        for name in ("len_L8_h1_sample", "cut_k31_sample_pieces5", "shared_4000_reads"):
            run_case(ka, ctx, oracle, bs.BY_NAME[name], tmp_path)
            assert search() == before, ("the search after constructing", name)
    finally:
        b.close()
        g.close()


# ---- (d) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["params_k32_h5", "cut_k31_P+k_pieces2", "shared_4000_reads"])
def test_no_false_negative_through_the_chain(ka, ctx, oracle, tmp_path, name):
    """Sequences -> kwage_make_bloom -> kwage_build_db -> the loader -> a search of every source sequence at t = 1: the
    sample's column is among the hits of every sequence that has a k-mer."""
    from test_builder import _device_build
    case = bs.BY_NAME[name]
    other = [bs.rand_seq(np.random.default_rng(99), 300)]
    blooms = [str(tmp_path / "other.bloom"), str(tmp_path / "sample.bloom")]
    device_file(ctx, oracle, other, case.k, case.num_hash, case.L, blooms[0])
    device_file(ctx, oracle, case.seqs, case.k, case.num_hash, case.L, blooms[1])
    db = str(tmp_path / "chain.db")
    _device_build(ka, ctx, blooms, (case.k, case.num_hash, case.L, 0), db)
    g = ka.Group(ctx, case.k, case.num_hash, case.L, 2)
    try:
        assert g.add_db_file(db) == (0, 2)
        g.finalize()
        b = ka.Batch(ctx, case.seqs)
        try:
            r = g.search(b, 1.0)
        finally:
            b.close()
    finally:
        g.close()
    counts = {s: len(oracle.unique_kmers(s, case.k)) for s in bs.distinct_seqs(case.seqs)}
    want = [counts[s] for s in case.seqs]
    assert r.num_query_kmer.tolist() == want and sum(want) > 0
    found = set(r.hits["query"][r.hits["column"] == 1].tolist())
    missing = [q for q, n in enumerate(want) if n and q not in found]
    assert not missing, (name, "queries that do not find their own sample", missing[:10])
