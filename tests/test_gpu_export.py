"""Export (include/kwage_amd.h: kwage_group_export_filters, its device and file forms; Group.export_filters,
Group.export_bloom_files, FileDatabase.export_samples, `kwage_dbtool extract`): listed columns of a RESIDENT group handed
back as whole Bloom filters, transposed on the device.

The expected filters come from code that existed before the export, never from it: Group.read_rows of all 2^L rows,
np.unpackbits(bitorder="little"), the listed columns, transposed and packed.  Every group carries a host or file block, a
live insert at a non-zero bit offset and a retired column, so that pads lie inside the row."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_IO, ERR_STATE = -1, -3, -6
K, NH = 15, 2
TILE_FILTERS = 1024                         # export.hip's ExportTile: TransposeTile<16, 8>::FILTERS


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


def filter_bytes(L):
    return max(1, (1 << L) // 8)


def random_filters(rng, L, n):
    return rng.integers(0, 256, size=(n, filter_bytes(L)), dtype=np.uint8)


class Mixed:
    """A group of `host` host-block columns at column 0 (pads up to the next 16-byte boundary behind them), a live insert
    of 5 filters and one of `live` more right behind it (bit offset 5), and one retired column of each kind; .bits is
    read_rows of every row unpacked (bool [2^L, span]), .valid the columns that hold a sample."""

    def __init__(self, ka, ctx, L, host=40, live=60, capacity=1024, finalize=True, seed=0):
        rng = np.random.default_rng([L, host, live, seed])
        self.L, self.nrows = L, 1 << L
        self.g = g = ka.Group(ctx, K, NH, L, capacity)
        image = rng.integers(0, 256, size=(self.nrows, (host + 7) // 8), dtype=np.uint8)
        assert g.add_columns(image, host) == 0
        self.first_live = g.insert_filters(random_filters(rng, L, 5))
        assert self.first_live % 128 == 0 and self.first_live >= host
        assert g.insert_filters(random_filters(rng, L, live)) == self.first_live + 5          # a non-zero bit offset
        self.retired = [host // 2, self.first_live + 2]
        g.retire_columns(self.retired)
        if finalize:
            g.finalize()
        self.refresh()

    def refresh(self):
        g = self.g
        self.bits = np.unpackbits(g.read_rows(np.arange(self.nrows)), axis=1, bitorder="little").astype(bool)
        self.valid = np.flatnonzero(g.real_columns())

    def expected(self, cols):
        """uint8 [n, filter bytes]: the listed columns as filters (for L < 3 the bits at and above 2^L are zero)"""
        return np.packbits(self.bits[:, np.asarray(cols, dtype=np.int64)].T, axis=1, bitorder="little")

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def mixed(ka, ctx):
    made = {}

    def get(L):
        if L not in made:
            made[L] = Mixed(ka, ctx, L)
        return made[L]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def wide(ka, ctx):
    """L = 10, 100 host columns, 5 + 2200 live ones: more than two tiles' worth of filters"""
    m = Mixed(ka, ctx, 10, host=100, live=2200, capacity=4096)
    yield m
    m.close()


def export_abi(g, cols, out_ptr, stride, staging=0, flags=0, ms=None):
    from kwage_amd.native import lib
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return lib().kwage_group_export_filters(g._h, cols.ctypes.data_as(C.POINTER(C.c_uint64)), cols.size, out_ptr, stride, staging, flags, ms)


# ------------------------------------------------------------------------------------------------------------------
# 1. shapes
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 5, 6, 10, 13])
def test_shapes(mixed, L, n):
    m = mixed(L)
    rng = np.random.default_rng([L, n])
    start = int(rng.integers(0, m.valid.size - n + 1))
    cols = m.valid[start:start + n]
    got = m.g.export_filters(cols)
    want = m.expected(cols)
    assert got.shape == (n, filter_bytes(L)) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if L < 3:
        assert not (got >> (1 << L)).any()              # one byte per filter, the bits at and above 2^L zero
    assert L < 5 or (want.any() and (want != 0xFF).any())


# ------------------------------------------------------------------------------------------------------------------
# 2. every bit offset
# ------------------------------------------------------------------------------------------------------------------

def test_every_bit_offset(wide):
    m = wide
    base = m.first_live + 5                             # 2200 consecutive valid columns from here on
    assert np.array_equal(m.valid[m.valid >= base], np.arange(base, base + 2200))
    for first in range(base, base + 161):
        for length in (1, 33, 128, 129):
            cols = np.arange(first, first + length)
            got = m.g.export_filters(cols)
            assert np.array_equal(got, m.expected(cols)), (first, length)


# ------------------------------------------------------------------------------------------------------------------
# 3. list shapes
# ------------------------------------------------------------------------------------------------------------------

def test_list_shapes(wide):
    m = wide
    v = m.valid
    host = v[v < 100]
    live = v[v >= m.first_live]
    across = np.stack([host[-20:], live[:20]], axis=1).ravel()          # alternating across the host block's alignment pad
    lists = {
        "ascending scattered": v[::7],
        "reversed": v[::-1][:300],
        "three times": np.array([v[11], v[40], v[11], v[500], v[11]]),
        "across the pad": across,
        "the last valid column": v[-1:],
        "two tiles and one": v[:2 * TILE_FILTERS + 1],
        "runs that repeat": np.concatenate([live[10:300], live[10:300], host[:30]]),
    }
    assert lists["two tiles and one"].size == 2049 and m.g.column_span - 8 < int(v[-1]) < m.g.column_span
    for name, cols in lists.items():
        got = m.g.export_filters(cols)
        want = m.expected(cols)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


# ------------------------------------------------------------------------------------------------------------------
# 4. chunks and strides
# ------------------------------------------------------------------------------------------------------------------

def test_chunks_and_strides(mixed):
    m = mixed(13)
    fb = filter_bytes(13)
    cols = np.concatenate([m.valid[3:60], m.valid[70:83]])
    n = cols.size
    assert n == 70
    want = m.expected(cols)
    for staging in (0, 4096, n):                        # one chunk, 58 bytes of every filter per chunk, one byte
        got = m.g.export_filters(cols, staging_bytes=staging)
        assert np.array_equal(got, want), staging
    for staging in (0, 4096):
        buf = np.full((n, fb + 24), 0xA5, dtype=np.uint8)
        out = m.g.export_filters(cols, out=buf[:, :fb], staging_bytes=staging)
        assert out.base is buf and np.array_equal(buf[:, :fb], want) and (buf[:, fb:] == 0xA5).all()
    # n = 1 with stride 0, into the middle of a buffer
    buf = np.full(fb + 64, 0xA5, dtype=np.uint8)
    assert export_abi(m.g, cols[:1], buf.ctypes.data + 32, 0) == 0
    assert np.array_equal(buf[32:32 + fb], want[0]) and (buf[:32] == 0xA5).all() and (buf[32 + fb:] == 0xA5).all()
    # filters of one byte, apart and pre-filled
    small = mixed(2)
    cols = small.valid[:9]
    buf = np.full((9, 3), 0xA5, dtype=np.uint8)
    small.g.export_filters(cols, out=buf[:, :1])
    assert np.array_equal(buf[:, :1], small.expected(cols)) and (buf[:, 1:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------------
# 5. device form
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [2, 6, 10, 13])
def test_device_form(ctx, mixed, L):
    import torch
    m = mixed(L)
    fb = filter_bytes(L)
    cols = np.concatenate([m.valid[50:20:-1], m.valid[60:101]])
    want = m.expected(cols)
    pitch = (fb + 3) // 4 * 4 + 8
    dev = torch.full((cols.size, pitch), 0xA5, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    out, ms = m.g.export_filters(cols, out=dev[:, :fb], timing=True)
    got = dev.cpu().numpy()
    assert np.array_equal(got[:, :fb], want), np.argwhere(got[:, :fb] != want)[:5]
    assert (got[:, fb:] == 0xA5).all() and ms > 0
    assert np.array_equal(m.g.export_filters(cols), got[:, :fb])
    host, ms = m.g.export_filters(cols, timing=True)
    assert ms > 0 and np.array_equal(host, want)


# ------------------------------------------------------------------------------------------------------------------
# 6. round trips
# ------------------------------------------------------------------------------------------------------------------

def test_round_trips(ka, ctx, mixed):
    import torch
    L = 10
    m = mixed(L)
    before = m.g.read_rows(np.arange(m.nrows))
    cols = np.concatenate([m.valid[5:45], m.valid[80:50:-1]])
    exported = m.g.export_filters(cols)
    for form in ("host", "device"):
        g2 = ka.Group(ctx, K, NH, L, 1024)
        try:
            rng = np.random.default_rng(5)
            assert g2.insert_filters(random_filters(rng, L, 3)) == 0
            bits = exported if form == "host" else torch.from_numpy(exported).to(torch.device("cuda", ctx.device))
            first = g2.insert_filters(bits)
            assert first == 3                           # a non-zero bit offset
            back = np.unpackbits(g2.read_rows(np.arange(m.nrows)), axis=1, bitorder="little").astype(bool)
            assert np.array_equal(back[:, first:first + cols.size], m.bits[:, cols]), form
            # what was just inserted from random bits comes back as those bits
            fresh = random_filters(rng, L, 37)
            at = g2.insert_filters(fresh)
            assert np.array_equal(g2.export_filters(np.arange(at, at + 37)), fresh)
        finally:
            g2.close()
    fs = ka.FilterSet.from_bits(ctx, K, NH, L, exported)
    try:
        assert np.array_equal(fs.bit_counts(), m.g.column_bits()[cols])
    finally:
        fs.close()
    assert np.array_equal(m.g.read_rows(np.arange(m.nrows)), before)          # the matrix is only read


# ------------------------------------------------------------------------------------------------------------------
# 7. lifecycle
# ------------------------------------------------------------------------------------------------------------------

def test_lifecycle(ka, ctx):
    m = Mixed(ka, ctx, 10, finalize=False, seed=7)
    try:
        g = m.g
        cols = m.valid[::-1][:80]
        want = m.expected(cols)
        assert np.array_equal(g.export_filters(cols), want)                 # before finalize ...
        g.finalize()
        assert np.array_equal(g.export_filters(cols), want)                 # ... and after: the same bytes
        gone = int(cols[7])
        g.retire_columns([gone])
        with pytest.raises(ka.KwageError) as e:
            g.export_filters(cols)
        assert e.value.code == ERR_ARG and "pad or retired" in str(e.value)
        rest = cols[cols != gone]
        assert np.array_equal(g.export_filters(rest), m.expected(rest))
        m.refresh()
        survivors = m.valid
        before = g.export_filters(survivors)
        assert np.array_equal(before, m.expected(survivors))
        new, _ = g.compact()
        assert np.array_equal(new[survivors], np.arange(survivors.size))
        assert np.array_equal(g.export_filters(new[survivors]), before)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. refusals write nothing
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(ka, ctx, mixed, tmp_path):
    import torch
    from kwage_amd import native
    from kwage_amd.native import lib
    L = 10
    m = mixed(L)
    g = m.g
    fb = filter_bytes(L)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    good = m.valid[:5].astype(np.uint64)
    buf = np.full((5, fb), 0xA5, dtype=np.uint8)
    dev = torch.full((5, fb + 4), 0xA5, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    ms = C.c_float(7.0)
    before = g.read_rows(np.arange(m.nrows))
    state = (g.column_span, g.num_columns)
    golden_db = os.path.join(GOLDEN, "multi", "dbs", "a", "k31_L10_h1.db")
    n_golden = native.DbHeader()
    native.check(lib().kwage_db_read_header(golden_db.encode(), C.byref(n_golden)))

    def u64(a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return a, a.ctypes.data_as(C.POINTER(C.c_uint64))

    def files_abi(group, cols, sources, paths):
        sc, keep = ka.Group._save_columns(cols, sources)
        arr = (C.c_char_p * max(len(paths), 1))(*[None if p is None else str(p).encode() for p in paths])
        return lib().kwage_group_export_bloom_files(group._h if group is not None else None, sc if cols is not None else None, arr, len(paths), 0, 0, C.byref(ms))

    def refused(rc, want=ERR_ARG, word=None):
        assert rc == want, (rc, lib().kwage_last_error())
        assert word is None or word in lib().kwage_last_error(), lib().kwage_last_error()
        assert (buf == 0xA5).all() and bool((dev == 0xA5).all()) and ms.value == 7.0
        assert os.listdir(str(out_dir)) == []
        assert (g.column_span, g.num_columns) == state

    host = lib().kwage_group_export_filters
    devf = lib().kwage_group_export_filters_device
    keep, gp = u64(good)
    refused(host(g._h, None, 5, buf.ctypes.data, fb, 0, 0, C.byref(ms)), word=b"NULL")
    refused(host(g._h, gp, 5, None, fb, 0, 0, C.byref(ms)), word=b"NULL")
    refused(host(None, gp, 5, buf.ctypes.data, fb, 0, 0, C.byref(ms)), word=b"NULL")
    refused(host(g._h, gp, 0, buf.ctypes.data, fb, 0, 0, C.byref(ms)), word=b"n is 0")
    refused(host(g._h, gp, 5, buf.ctypes.data, fb - 1, 0, 0, C.byref(ms)), word=b"smaller than a filter")
    for bad, word in (([int(good[0]), g.column_span], b"beyond the span"), ([int(good[0]), 1 << 40], b"beyond the span"),
                      ([int(good[1]), m.retired[0]], b"pad or retired"), ([m.retired[1]], b"pad or retired"),
                      ([int(good[0]), 101], b"pad or retired")):                    # (101: a pad behind the host block)
        k2, p2 = u64(bad)
        refused(host(g._h, p2, len(bad), buf.ctypes.data, fb, 0, 0, C.byref(ms)), word=word)
        refused(devf(g._h, p2, len(bad), dev.data_ptr(), dev.stride(0), 0, C.byref(ms)), word=word)
        refused(files_abi(g, bad, [(golden_db, 0)] * len(bad), [out_dir / ("x%d.bloom" % i) for i in range(len(bad))]), word=word)
    refused(devf(g._h, gp, 5, None, dev.stride(0), 0, C.byref(ms)), word=b"NULL")
    refused(devf(g._h, gp, 5, dev.data_ptr() + 2, dev.stride(0), 0, C.byref(ms)), word=b"multiples of 4")
    refused(devf(g._h, gp, 5, dev.data_ptr(), dev.stride(0) + 2, 0, C.byref(ms)), word=b"multiples of 4")
    refused(devf(g._h, gp, 5, dev.data_ptr(), fb - 4, 0, C.byref(ms)), word=b"smaller than a filter")
    refused(devf(g._h, gp, 0, dev.data_ptr(), dev.stride(0), 0, C.byref(ms)), word=b"n is 0")
    # the file form
    paths = [out_dir / ("s%d.bloom" % i) for i in range(5)]
    src = [(golden_db, i) for i in range(5)]
    refused(files_abi(None, good, src, paths), word=b"NULL")
    refused(files_abi(g, good, src, []), word=b"n is 0")
    refused(files_abi(g, good, src[:4] + [None], paths), word=b"neither")
    refused(files_abi(g, good, src[:4] + [(golden_db, n_golden.num_filter)], paths), word=b"has no column")
    refused(files_abi(g, good, src, paths[:4] + [None]), word=b"path")
    refused(files_abi(g, good, src[:4] + [(str(tmp_path / "missing.db"), 0)], paths), want=ERR_IO)
    refused(files_abi(g, good, src[:4] + [{"run_accession": "not an accession"}], paths))
    sc, _ = ka.Group._save_columns(good, src)
    refused(lib().kwage_group_export_bloom_files(g._h, sc, None, 5, 0, 0, C.byref(ms)), word=b"NULL")
    # a sparse group
    sparse = ka.Group.sparse(ctx, K, NH, L, 1024, np.arange(0, m.nrows, 2))
    try:
        image = np.full((m.nrows // 2, 2), 0x5A, dtype=np.uint8)
        assert sparse.add_columns(image, 16) == 0
        sparse.finalize()
        c2, p2 = u64([0, 1, 2, 3, 4])
        refused(host(sparse._h, p2, 5, buf.ctypes.data, fb, 0, 0, C.byref(ms)), word=b"sparse")
        refused(devf(sparse._h, p2, 5, dev.data_ptr(), dev.stride(0), 0, C.byref(ms)), word=b"sparse")
        refused(files_abi(sparse, [0, 1, 2, 3, 4], src, paths), word=b"sparse")
    finally:
        sparse.close()
    # between submit and collect
    rng = np.random.default_rng(8)
    b = ka.Batch(ctx, ["".join(rng.choice(list("ACGT"), size=40)) for _ in range(10)])
    try:
        pending = g.submit(b, 1.0)
        rcs = (host(g._h, gp, 5, buf.ctypes.data, fb, 0, 0, C.byref(ms)), devf(g._h, gp, 5, dev.data_ptr(), dev.stride(0), 0, C.byref(ms)),
               files_abi(g, good, src, paths))
        err = lib().kwage_last_error()
        pending.collect()
        assert rcs == (ERR_STATE, ERR_STATE, ERR_STATE) and b"pending" in err
        refused(ERR_ARG)
    finally:
        b.close()
    # a destination directory that does not exist: none of the n files is written ...
    there = [out_dir / "a.bloom", out_dir / "b.bloom", tmp_path / "no_such_dir" / "c.bloom", out_dir / "d.bloom", out_dir / "e.bloom"]
    refused(files_abi(g, good, src, there), want=ERR_IO)
    # ... and a destination that existed before a failing call keeps its bytes
    (out_dir / "a.bloom").write_bytes(b"as it was")
    assert files_abi(g, good, src, there) == ERR_IO
    assert os.listdir(str(out_dir)) == ["a.bloom"] and (out_dir / "a.bloom").read_bytes() == b"as it was"
    os.remove(str(out_dir / "a.bloom"))
    # and the group still exports, unchanged
    assert np.array_equal(g.read_rows(np.arange(m.nrows)), before)
    assert host(g._h, gp, 5, buf.ctypes.data, fb, 0, 0, None) == 0 and np.array_equal(buf, m.expected(good))


# ------------------------------------------------------------------------------------------------------------------
# 9. `.bloom` files
# ------------------------------------------------------------------------------------------------------------------

def test_bloom_files_synthetic(ka, ctx, oracle, tmp_path):
    from kwage_amd.native import lib, check
    from kwage_amd import native
    L, n = 11, 70
    rng = np.random.default_rng(9)
    src_dir, out_dir = tmp_path / "src", tmp_path / "out"
    src_dir.mkdir()
    out_dir.mkdir()
    filters = random_filters(rng, L, n)
    paths = []
    for j in range(n):
        fi = oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (j + 1)), experiment_title="title %d" % j, number_of_bases=1000 + j,
                               sample_attributes=[("tag", "value %d" % j)] if j % 2 else [], date=(j % 28 + 1, j % 12 + 1, 2000 + j))
        p = str(src_dir / ("f%03d.bloom" % j))
        oracle.write_bloom(p, K, L, NH, fi, filters[j])
        paths.append(p)
    db = str(tmp_path / "seventy.db")
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    params = native.Params(K, NH, L, 0)
    check(lib().kwage_build_db(ctx._h, db.encode(), C.byref(params), arr, n, None))
    g = ka.Group(ctx, K, NH, L, 1024)
    g2 = ka.Group(ctx, K, NH, L, 1024)
    try:
        first, nf = g.add_db_file(db)
        assert (first, nf) == (0, n)
        g.finalize()
        outs = [str(out_dir / ("f%03d.bloom" % j)) for j in range(n)]
        g.export_bloom_files(list(range(n)), [(db, j) for j in range(n)], outs, staging_bytes=4096)
        assert sorted(os.listdir(str(out_dir))) == sorted(os.path.basename(p) for p in outs)          # no temporary file is left
        for a, b in zip(paths, outs):
            assert open(a, "rb").read() == open(b, "rb").read(), b
        assert g2.insert_filters(random_filters(rng, L, 3)) == 0
        at = g2.insert_bloom_files(outs[::-1])
        back = g2.export_filters(np.arange(at, at + n))
        assert np.array_equal(back, filters[::-1])
        rows = np.unpackbits(g2.read_rows(np.arange(1 << L)), axis=1, bitorder="little")[:, at:at + n]
        assert np.array_equal(rows.T, np.unpackbits(filters[::-1], axis=1, bitorder="little"))
    finally:
        g.close()
        g2.close()


def test_bloom_files_of_the_reference_made_database(ka, ctx, oracle, tmp_path):
    from kwage_amd.native import lib, check
    from kwage_amd import native
    golden = os.path.join(GOLDEN, "basic", "db", "basic.db")
    ref = oracle.read_db(golden)
    h = ref.header
    n = h.num_filter
    g = ka.Group(ctx, h.kmer_len, h.num_hash, h.log_2_filter_len, n)
    try:
        assert g.add_db_file(golden) == (0, n)
        g.finalize()
        outs = [str(tmp_path / ("c%03d.bloom" % j)) for j in range(n)]
        g.export_bloom_files(list(range(n)), [(golden, j) for j in range(n)], outs)
        cols = np.unpackbits(ref.rows, axis=1, bitorder="little")[:, :n]
        for j in (0, 9, n - 1):
            prm, crc, fi, bits = oracle.read_bloom(outs[j])
            assert prm == (h.kmer_len, h.log_2_filter_len, h.num_hash, h.hash_func)
            assert np.array_equal(np.unpackbits(bits, bitorder="little"), cols[:, j])
        rebuilt = str(tmp_path / "rebuilt.db")
        arr = (C.c_char_p * n)(*[p.encode() for p in outs])
        params = native.Params(h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func)
        check(lib().kwage_build_db(ctx._h, rebuilt.encode(), C.byref(params), arr, n, None))
        a, b = open(golden, "rb").read(), open(rebuilt, "rb").read()
        assert a[:h.info_start] == b[:h.info_start]     # the header with its CRC and the whole slice block
        again = oracle.read_db(rebuilt)
        for j in range(n):
            x, y = ref.info(j), again.info(j)
            assert dict(x.sample_attributes) == dict(y.sample_attributes) and len(x.sample_attributes) == len(y.sample_attributes)
            x.sample_attributes = y.sample_attributes = []
            assert x == y, j
        # an `info` source: the record is serialized from the fields given
        info = {"run_accession": "SRR77", "experiment_accession": "SRX5", "experiment_title": "a title", "sample_taxa": "9606",
                "attribute_tags": ["tissue"], "attribute_values": ["leaf"], "num_attributes": 1, "number_of_spots": 12, "number_of_bases": 3400,
                "day": 3, "month": 4, "year": 2019}
        one = str(tmp_path / "info.bloom")
        g.export_bloom_files([5], [info], [one])
        prm, crc, fi, bits = oracle.read_bloom(one)
        assert np.array_equal(np.unpackbits(bits, bitorder="little"), cols[:, 5])
        assert fi == oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR77"), experiment_accession=oracle.str_to_accession("SRX5"),
                                       experiment_title="a title", sample_taxa="9606", sample_attributes=[("tissue", "leaf")], number_of_spots=12,
                                       number_of_bases=3400, date=(3, 4, 2019))
    finally:
        g.close()


def test_more_files_than_are_written_side_by_side(wide, oracle, tmp_path):
    """600 files: the file form goes through its list 256 files at a time, and renames all of them at the end"""
    import zlib
    m = wide
    cols = np.concatenate([m.valid[:400], m.valid[:-201:-1]])
    n = cols.size
    assert n == 600
    want = m.expected(cols)
    outs = [str(tmp_path / ("s%04d.bloom" % i)) for i in range(n)]
    m.g.export_bloom_files(cols, [{"run_accession": "SRR%d" % (i + 1)} for i in range(n)], outs, staging_bytes=1 << 14)
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in outs)
    for i in (0, 1, 255, 256, 257, 511, 512, 513, 599):
        prm, crc, fi, bits = oracle.read_bloom(outs[i])
        assert prm == (K, m.L, NH, 0) and crc == zlib.crc32(bits.tobytes()) & 0xFFFFFFFF
        assert np.array_equal(bits, want[i]), i
        assert fi == oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (i + 1)))
        assert os.path.getsize(outs[i]) == 21 + len(oracle.pack_filter_info(fi)) + bits.size
    # a failure in the last batch leaves none of the earlier batches' files either
    gone = tmp_path / "gone"
    gone.mkdir()
    outs = [str(gone / ("s%04d.bloom" % i)) for i in range(n - 1)] + [str(tmp_path / "no_such_dir" / "x.bloom")]
    with pytest.raises(Exception) as e:
        m.g.export_bloom_files(cols, [{"run_accession": "SRR%d" % (i + 1)} for i in range(n)], outs)
    assert e.value.code == ERR_IO and os.listdir(str(gone)) == []


# ------------------------------------------------------------------------------------------------------------------
# 10. kwage_dbtool extract
# ------------------------------------------------------------------------------------------------------------------

def test_dbtool_extract(ka, ctx, oracle, tmp_path):
    from kwage_amd import native
    tool = native.KWAGE_DBTOOL_BIN
    golden = os.path.join(GOLDEN, "k32")
    db = os.path.join(golden, "k32.db")
    ref = oracle.read_db(db)
    h = ref.header
    n = h.num_filter
    accs = [ref.info(j).csv_string() for j in range(n)]
    assert len(set(accs)) == n

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    # what Group.export_bloom_files writes for the same columns
    lib_dir = tmp_path / "lib"
    lib_dir.mkdir()
    g = ka.Group(ctx, h.kmer_len, h.num_hash, h.log_2_filter_len, n)
    try:
        assert g.add_db_file(db) == (0, n)
        g.finalize()
        g.export_bloom_files(list(range(n)), [(db, j) for j in range(n)], [str(lib_dir / (a + ".bloom")) for a in accs])
    finally:
        g.close()
    every, two, none = tmp_path / "every", tmp_path / "two", tmp_path / "none"
    none.mkdir()
    r = run("extract", str(every), db)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(str(every))) == sorted(a + ".bloom" for a in accs)
    for a in accs:
        assert (every / (a + ".bloom")).read_bytes() == (lib_dir / (a + ".bloom")).read_bytes(), a
    r = run("extract", str(two), db, accs[6], accs[1])
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(str(two))) == sorted([accs[1] + ".bloom", accs[6] + ".bloom"])
    for a in (accs[1], accs[6]):
        assert (two / (a + ".bloom")).read_bytes() == (lib_dir / (a + ".bloom")).read_bytes(), a
    r = run("extract", str(none), db, accs[0], "SRR77777")
    assert r.returncode == 1 and "SRR77777" in r.stderr and os.listdir(str(none)) == []
    # build over the extracted files: a database that answers as the golden one does
    built = tmp_path / "built"
    built.mkdir()
    r = run("build", str(built / "k32.db"), str(h.kmer_len), str(h.log_2_filter_len), str(h.num_hash), *[str(every / (a + ".bloom")) for a in accs])
    assert r.returncode == 0, r.stderr
    assert (built / "k32.db").read_bytes()[:h.info_start] == open(db, "rb").read()[:h.info_start]
    case = [c for c in json.load(open(os.path.join(GOLDEN, "manifest.json")))["cases"] if c["name"] == "k32" and c["expected"] == "expected_t1.0.csv"][0]
    args = [native.KWAGE_BIN, "-d", str(built)]
    for q in case["queries"]:
        args += ["-i", q]
    args += ["-t", case["threshold"], "--o.csv"] + case["cmdline"]
    r = subprocess.run(args, cwd=golden, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    got, exp = oracle.parse_csv(r.stdout.decode("latin-1")), oracle.parse_csv(open(os.path.join(golden, case["expected"]), encoding="latin-1").read())
    assert list(got) == list(exp) and all(sorted(got[q]) == sorted(exp[q]) for q in exp)


# ------------------------------------------------------------------------------------------------------------------
# 11. FileDatabase.export_samples
# ------------------------------------------------------------------------------------------------------------------

def test_file_database_export_samples(ka, ctx, oracle, tmp_path):
    dbs = os.path.join(GOLDEN, "multi", "dbs")
    rng = np.random.default_rng(12)
    fresh = "".join(rng.choice(list("ACGT"), size=500))
    out_dir = tmp_path / "samples"
    db = ka.FileDatabase(ctx, [dbs], headroom=64)
    try:
        src = oracle.read_db(db.files[0])
        h = src.header
        file_acc = src.info(2).csv_string()
        gi, col = db.add_sample("SRR9999001", [fresh])
        p = db.groups[gi].params
        with pytest.raises(KeyError) as e:
            db.export_samples([file_acc, "SRR4040404"], str(out_dir))
        assert "SRR4040404" in str(e.value) and not out_dir.exists()
        written = db.export_samples(["SRR9999001", file_acc], str(out_dir))
        assert sorted(written) == sorted(str(out_dir / (a + ".bloom")) for a in ("SRR9999001", file_acc))
        assert sorted(os.listdir(str(out_dir))) == sorted(os.path.basename(w) for w in written)
        # the live sample: the exact k-mer set of its sequence, and a record that carries the accession only
        prm, crc, fi, bits = oracle.read_bloom(str(out_dir / "SRR9999001.bloom"))
        assert prm == (p.kmer_len, p.log_2_filter_len, p.num_hash, p.hash_func)
        assert np.array_equal(bits, oracle.bloom_bits_from_sequences([fresh], p.kmer_len, p.num_hash, p.log_2_filter_len))
        assert fi == oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR9999001"))
        # the file sample: its column of its file, the record of its file
        prm, crc, fi, bits = oracle.read_bloom(str(out_dir / (file_acc + ".bloom")))
        assert prm == (h.kmer_len, h.log_2_filter_len, h.num_hash, h.hash_func)
        assert np.array_equal(np.unpackbits(bits, bitorder="little"), np.unpackbits(src.rows, axis=1, bitorder="little")[:, 2])
        want = src.info(2)
        assert dict(fi.sample_attributes) == dict(want.sample_attributes)
        fi.sample_attributes = want.sample_attributes = []
        assert fi == want
    finally:
        db.close()
