"""kwage_filterset (include/kwage_amd.h): Bloom filters turned into ascending row lists on the device -- the extraction
alone.  Expected lists are np.flatnonzero of the bits the test itself made (from_bits) or of the column of the host image
the test itself loaded (from_columns); every comparison is exact integer equality.

The scan of the block sums (filter_scan_kernel) has three levels: within a wave, across the waves of its one workgroup,
and across that workgroup's rounds of 256 block sums.  A block sum covers 256 words of 64 rows, so a filter of 2^24 rows
is 1024 block sums = 4 rounds: L = 24 crosses every level, and the sets below hold several filters on top of that."""
import ctypes as C

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


def make_group(ka, ctx, rng, k, num_hash, L, files_nf, density):
    """A group of several 'files' (add_columns) with garbage in the pad bits of every image, built the way
    tests/test_gpu_scores.py builds its groups.  Returns (group, [(first_column, image, nf)])."""
    g = ka.Group(ctx, k, num_hash, L, sum(nf + 128 for nf in files_nf))
    files = []
    for nf in files_nf:
        bits = rng.random((1 << L, nf)) < density
        width = (nf + 7) // 8 + 3
        img = np.zeros((1 << L, width * 8), dtype=bool)
        img[:, :nf] = bits
        img[:, nf:] = rng.random((1 << L, width * 8 - nf)) < 0.5      # pad bits: garbage
        packed = np.packbits(img, axis=1, bitorder="little")
        first = g.add_columns(packed, nf)
        files.append((first, np.ascontiguousarray(packed), nf))
    g.finalize()
    return g, files


def patterns(rng, L):
    """[(name, uint8 bit vector of max(1, 2^L / 8) bytes)]: two full filters around an empty one, then the rest."""
    nrows = 1 << L
    nbytes = max(1, nrows // 8)

    def pack(bits):
        v = np.packbits(bits, bitorder="little")
        out = np.zeros(nbytes, dtype=np.uint8)
        out[:v.size] = v
        if nrows < 8:
            out[0] |= np.uint8((0xFF << nrows) & 0xA5 & 0xFF)       # bits at or beyond 2^L: garbage, to be ignored
        return out
    every_other = np.zeros(nrows, dtype=bool)
    for w0 in range(0, nrows, 128):
        every_other[w0:w0 + 64] = True
    first = np.zeros(nrows, dtype=bool)
    first[0] = True
    last = np.zeros(nrows, dtype=bool)
    last[-1] = True
    return [("full", pack(np.ones(nrows, dtype=bool))), ("empty", pack(np.zeros(nrows, dtype=bool))), ("full", pack(np.ones(nrows, dtype=bool))),
            ("first", pack(first)), ("last", pack(last)), ("every other word", pack(every_other)), ("random", pack(rng.random(nrows) < 0.5))]


@pytest.mark.parametrize("L", [0, 1, 2, 3, 5, 6, 7, 13, 14, 15, 22, 24])
def test_from_bits_rows_are_flatnonzero(ka, ctx, L):
    rng = np.random.default_rng(900 + L)
    pats = patterns(rng, L)
    bits = np.stack([v for _, v in pats])
    fs = ka.FilterSet.from_bits(ctx, 21, 2, L, bits)
    try:
        assert len(fs) == len(pats)
        counts = fs.bit_counts()
        for i, (name, v) in enumerate(pats):
            exp = np.flatnonzero(np.unpackbits(v, bitorder="little")[:1 << L]).astype(np.uint32)
            got = fs.rows(i)               # (read through the device's own prefix entry, which must equal the sum of the counts before it)
            assert counts[i] == exp.size, (L, name, int(counts[i]), exp.size)
            assert got.dtype == np.uint32 and np.array_equal(got, exp), (L, name, got[:8], exp[:8])
        assert counts[0] == 1 << L and counts[1] == 0 and counts[2] == 1 << L
    finally:
        fs.close()


def test_a_strided_source_and_an_empty_set(ka, ctx):
    from kwage_amd.native import lib, check, Params
    L = 9
    rng = np.random.default_rng(3)
    wide = rng.integers(0, 256, size=(5, 64 + 24), dtype=np.uint8)          # filters of 64 bytes, 88 bytes apart
    p = Params(21, 1, L, 0)
    h = C.c_void_p()
    check(lib().kwage_filterset_from_bits(ctx._h, C.byref(p), wide.ctypes.data, wide.strides[0], 5, C.byref(h)))
    fs = ka.FilterSet(ctx, p, h)
    try:
        for i in range(5):
            assert np.array_equal(fs.rows(i), np.flatnonzero(np.unpackbits(wide[i, :64], bitorder="little")))
    finally:
        fs.close()
    empty = ka.FilterSet.from_bits(ctx, 21, 1, L, np.zeros((0, 64), dtype=np.uint8))
    try:
        assert len(empty) == 0 and empty.bit_counts().size == 0
    finally:
        empty.close()


@pytest.mark.parametrize("L", [4, 6, 10])
def test_from_columns_equals_the_images_columns(ka, ctx, L):
    rng = np.random.default_rng(40 + L)
    nfs = [77, 21]
    g, files = make_group(ka, ctx, rng, 21, 3, L, nfs, 0.4)
    try:
        (f0, img0, nf0), (f1, img1, nf1) = files
        # bit 0 and bit 7 of a byte, the first and last real column of each file, a column twice
        cols = [f0 + 0, f0 + 7, f0 + 8, f0 + 15, f0 + nf0 - 1, f1 + 0, f1 + 5, f1 + nf1 - 1, f0 + 7]
        fs = ka.FilterSet.from_columns(g, cols)
        try:
            counts = fs.bit_counts()
            for i, c in enumerate(cols):
                first, img, _ = files[0] if c < f1 else files[1]
                lc = c - first
                exp = np.flatnonzero((img[:, lc // 8] >> (lc % 8)) & 1).astype(np.uint32)
                assert np.array_equal(fs.rows(i), exp) and counts[i] == exp.size, (L, c)
            assert np.array_equal(fs.rows(1), fs.rows(8))
        finally:
            fs.close()
        none = ka.FilterSet.from_columns(g, [])
        assert len(none) == 0
        none.close()
    finally:
        g.close()


def test_refusals_write_nothing(ka, ctx):
    from kwage_amd.native import lib, Params
    rng = np.random.default_rng(8)
    L = 8
    g, files = make_group(ka, ctx, rng, 21, 2, L, [13, 9], 0.5)
    (f0, img0, nf0), (f1, img1, nf1) = files
    span = g.column_span
    listed = np.arange(0, 1 << L, 3, dtype=np.uint32)
    sparse = ka.Group.sparse(ctx, 21, 2, L, 256, listed)
    sparse.add_columns(np.ascontiguousarray(img0[listed]), nf0)
    sparse.finalize()
    unfinished = ka.Group(ctx, 21, 2, L, 256)
    unfinished.add_columns(img0, nf0)
    SENTINEL = 0x1234

    def from_columns(group, cols):
        h = C.c_void_p(SENTINEL)
        arr = np.asarray(cols, dtype=np.uint64)
        rc = lib().kwage_filterset_from_columns(group._h, arr.ctypes.data, arr.size, C.byref(h))
        return rc, h.value
    try:
        for what, group, cols, code in (("a pad column behind the first file", g, [f0, f0 + nf0], -1),
                                        ("a pad column before the second file", g, [f1 - 1], -1),
                                        ("a column at the span", g, [f0, span], -1),
                                        ("a column beyond the span", g, [span + 5], -1),
                                        ("a sparse group", sparse, [0], -1),
                                        ("an unfinalized group", unfinished, [0], -6)):
            rc, h = from_columns(group, cols)
            assert rc == code and h == SENTINEL, (what, rc, h)
            assert lib().kwage_last_error(), what
        # 2^32 rows: refused before the bits are read (one byte stands in for them)
        h = C.c_void_p(SENTINEL)
        p = Params(21, 2, 32, 0)
        one = np.zeros(1, dtype=np.uint8)
        assert lib().kwage_filterset_from_bits(ctx._h, C.byref(p), one.ctypes.data, 1, 1, C.byref(h)) == -1 and h.value == SENTINEL
        assert b"2^32" in lib().kwage_last_error()
        # and the group still answers
        fs = ka.FilterSet.from_columns(g, [f0])
        assert np.array_equal(fs.rows(0), np.flatnonzero(img0[:, 0] & 1))
        fs.close()
    finally:
        unfinished.close()
        sparse.close()
        g.close()
