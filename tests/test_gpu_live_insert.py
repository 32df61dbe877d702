"""Live insert (include/kwage_amd.h: kwage_group_insert_filters / _device / _bloom_files, kwage_group_retire_columns): whole
Bloom filters become new columns of a RESIDENT group, before and after finalize, and withdrawn columns become pad columns.

The expected matrix is numpy's: the filters' bytes through np.unpackbits(..., bitorder="little") and a transpose, placed at
first_column of a bool image (class Image).  Expected search results are the CPU oracle's on that image
(kwage_oracle.search_image, bloom_bits_from_sequences) -- never the code under test; every comparison is exact equality.
A second witness is a COLD group given the same image through kwage_group_add_columns: same span, rows and results.

Two things the engine decides differently from what one might expect, and the tests say so where they meet them:
  - kwage_group_read_rows returns row_bytes bytes of a row, so the bytes between row_bytes and the stride are made visible
    by adding one-column blocks behind the insert (each starts on the next 16-byte boundary and writes one byte there):
    every byte up to the stride except those written bytes themselves is then compared with zero;
  - the gather kernel of a search is chosen from the group's row STRIDE (engine.hip launch_search_stage:
    units_per_row = stride / 16), i.e. from its capacity, not from how much of a row is in use: growing a group by
    inserts never changes search_kernel (test_across_the_row_widths_of_the_kernel_table)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
# (the expected matrix and the comparisons against it live in tests/group_model.py, which the model-based tests share)
from group_model import (Image, check_all_forms, check_rows, columns_of, oracle_counts, oracle_hits, random_dna, random_filters,     # noqa: F401
                         same_state, state_of)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
FILTERS_PER_TILE = 1024           # insert.hip InsertTile = TransposeTile<16, 8>: 32 words of 32 columns


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


# ------------------------------------------------------------------------------------------------------------------
# the numpy side
# ------------------------------------------------------------------------------------------------------------------

def check_zero_to_the_stride(ka, g, image):
    """(un-finalized groups) One-column blocks behind everything make the rest of the row visible: see the module's text."""
    nrows = image.bits.shape[0]
    wrote = []
    one = np.zeros((nrows, 1), dtype=np.uint8)
    while (g.row_bytes + 15) // 16 * 16 < g.row_stride:
        first = g.add_columns(one, 1)
        wrote.append(first // 8)
    got = g.read_rows(np.arange(nrows))
    assert np.array_equal(got[:, :image.span // 8], image.packed())
    rest = got[:, image.span // 8:]
    assert not rest.any(), (image.span // 8, np.argwhere(rest)[:5])
    return len(wrote)


# ------------------------------------------------------------------------------------------------------------------
# 1. shapes
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [0, 1, 2, 3, 5, 6, 10, 13])
def test_shapes(ka, ctx, L):
    ns = [1, 7, 8, 9, 31, 32, 33, 127, 128, 129] + ([FILTERS_PER_TILE - 1, FILTERS_PER_TILE, FILTERS_PER_TILE + 1] if L == 10 else [])
    rng = np.random.default_rng(100 + L)
    nrows = 1 << L
    rows = None if L < 13 else np.sort(rng.choice(nrows, size=4096, replace=False))
    for n in ns:
        filters = random_filters(rng, L, n)
        image = Image(L)
        image.put(0, columns_of(filters, L))
        g = ka.Group(ctx, 21, 2, L, n + 200)
        try:
            assert g.insert_filters(filters) == 0
            check_rows(g, image, rows)
            if L <= 10:
                assert check_zero_to_the_stride(ka, g, image) >= 1, (L, n)
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. every bit offset
# ------------------------------------------------------------------------------------------------------------------

def test_every_bit_offset(ka, ctx):
    L = 6
    rng = np.random.default_rng(2)
    for s in range(0, 33):
        filters = random_filters(rng, L, s + 40)
        image = Image(L)
        image.put(0, columns_of(filters, L))
        two, one = ka.Group(ctx, 21, 2, L, 300), ka.Group(ctx, 21, 2, L, 300)
        try:
            if s:
                assert two.insert_filters(filters[:s]) == 0
                head = Image(L)
                head.put(0, columns_of(filters[:s], L))
                check_rows(two, head)                                  # the first block alone, zero above its tail
            assert two.insert_filters(filters[s:]) == s
            assert one.insert_filters(filters) == 0
            check_rows(two, image)
            check_rows(one, image)
            assert np.array_equal(two.read_rows(np.arange(1 << L)), one.read_rows(np.arange(1 << L)))
            assert np.array_equal(two.real_columns(), one.real_columns())
        finally:
            two.close()
            one.close()


def test_one_at_a_time_equals_one_call_equals_a_cold_group(ka, ctx):
    L, n = 10, 200
    rng = np.random.default_rng(22)
    filters = random_filters(rng, L, n)
    image = Image(L)
    image.put(0, columns_of(filters, L))
    single, whole, cold = (ka.Group(ctx, 21, 2, L, 1000) for _ in range(3))
    try:
        for i in range(n):
            assert single.insert_filters(filters[i:i + 1]) == i
        assert whole.insert_filters(filters) == 0
        assert cold.add_columns(image.packed(), n) == 0
        for g in (single, whole, cold):
            check_rows(g, image)
        assert single.column_span == whole.column_span == cold.column_span == 200 and single.row_bytes == 25
    finally:
        for g in (single, whole, cold):
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. neighbours
# ------------------------------------------------------------------------------------------------------------------

def test_neighbours_keep_their_bytes_and_pads_stay_pads(ka, ctx, oracle):
    k, nh, L = 15, 1, 8
    rng = np.random.default_rng(3)
    file_cols = rng.random((1 << L, 13)) < 0.5
    host = np.packbits(np.concatenate([file_cols, np.ones((1 << L, 3), dtype=bool)], axis=1), axis=1, bitorder="little")     # pad bits of the last byte: all set
    assert host.shape[1] == 2 and (host[:, 1] >> 5 == 7).all()
    filters = random_filters(rng, L, 50)
    image = Image(L)
    image.put(0, file_cols)
    g = ka.Group(ctx, k, nh, L, 1000)
    try:
        assert g.add_columns(host, 13) == 0
        g.finalize()
        first = g.insert_filters(filters)
        assert first == 128                                          # the next 16-byte boundary of the row
        image.put(first, columns_of(filters, L))
        got = g.read_rows(np.arange(1 << L))
        assert np.array_equal(got[:, :2], host)                      # the file block's bytes, pad garbage included
        assert not got[:, 2:16].any() and np.array_equal(got[:, 16:], image.packed()[:, 16:])
        assert g.column_span == image.span and g.num_columns == 63
        queries = [random_dna(rng, 16) for _ in range(12)] + [random_dna(rng, 15), "ACGT"]
        check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [0, 12, first, first + 49])
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. forms
# ------------------------------------------------------------------------------------------------------------------

def test_host_stride_and_device_form(ka, ctx):
    import torch
    from kwage_amd.native import lib
    L = 9
    rng = np.random.default_rng(4)
    wide = rng.integers(0, 256, size=(37, 64 + 24), dtype=np.uint8)          # filters of 64 bytes, 88 bytes apart
    more = random_filters(rng, L, 70)
    padded = rng.integers(0, 256, size=(9, 72), dtype=np.uint8)              # device rows 72 bytes apart
    image = Image(L)
    image.put(0, columns_of(np.ascontiguousarray(wide[:, :64]), L))
    image.put(37, columns_of(more, L))
    image.put(107, columns_of(np.ascontiguousarray(padded[:, :64]), L))
    g = ka.Group(ctx, 21, 2, L, 400)
    try:
        assert g.insert_filters(wide) == 0
        dev = torch.device("cuda", ctx.device)
        assert g.insert_filters(torch.from_numpy(more).to(dev)) == 37
        assert g.insert_filters(torch.from_numpy(padded).to(dev)) == 107
        check_rows(g, image)
        # timing: the insert kernels' HIP-event duration
        first, ms = C.c_uint64(), C.c_float(-1)
        one = random_filters(rng, L, 1)
        assert lib().kwage_group_insert_filters(g._h, one.ctypes.data, 0, 1, ka.SEARCH_TIMING, C.byref(first), C.byref(ms)) == 0
        assert first.value == 116 and 0 < ms.value < 100
        g._real.append((116, 1))
        image.put(116, columns_of(one, L))
        check_rows(g, image)
    finally:
        g.close()


def test_bloom_files_equal_build_db_and_load(ka, ctx, oracle, tmp_path):
    from kwage_amd.native import lib, check, Params
    k, nh, L, n = 21, 3, 12, 45
    rng = np.random.default_rng(44)
    filters = random_filters(rng, L, n)
    paths = []
    for i in range(n):
        p = str(tmp_path / ("s%03d.bloom" % i))
        oracle.write_bloom(p, k, L, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (7000 + i))), filters[i])
        paths.append(p)
    image = Image(L)
    image.put(0, columns_of(filters, L))
    db = str(tmp_path / "built.db")
    prm = Params(k, nh, L, 0)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    check(lib().kwage_build_db(ctx._h, db.encode(), C.byref(prm), arr, n, None))
    live, loaded = ka.Group(ctx, k, nh, L, 500), ka.Group(ctx, k, nh, L, 500)
    try:
        assert live.insert_bloom_files(paths) == 0
        assert loaded.add_db_file(db) == (0, n)
        check_rows(live, image)
        check_rows(loaded, image)
        assert np.array_equal(live.read_rows(np.arange(1 << L)), loaded.read_rows(np.arange(1 << L)))
        assert live.insert_bloom_files(paths[:3]) == n              # and the next call continues at the tail
        image.put(n, columns_of(filters[:3], L))
        check_rows(live, image)
    finally:
        live.close()
        loaded.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. searchable at once, before and after finalize
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """40 samples of 300 bases and one new one, with queries cut from both (shared by the cases below, never changed)."""
    rng = np.random.default_rng(5)
    samples = [random_dna(rng, 300) for _ in range(40)]
    new = random_dna(rng, 300)
    queries = [samples[3][10:110], samples[17][150:290], new[20:140], new[5:60] + samples[30][5:60], random_dna(rng, 80),
               samples[39][0:40] + "N" + new[100:160], "ACGTACGT"]
    return samples, new, queries


@pytest.mark.parametrize("when", ["after finalize", "before finalize"])
@pytest.mark.parametrize("nh", [1, 3, 5])
def test_searchable_at_once(ka, ctx, oracle, planted, nh, when):
    k, L = 15, 13
    samples, new, queries = planted
    rng = np.random.default_rng(50 + nh)
    old = np.stack([oracle.bloom_bits_from_sequences([s], k, nh, L) for s in samples])
    fresh = oracle.bloom_bits_from_sequences([new], k, nh, L)[None, :]
    host = np.packbits(np.concatenate([columns_of(old, L), rng.random((1 << L, 24)) < 0.5], axis=1), axis=1, bitorder="little")      # 40 columns, garbage behind
    image = Image(L)
    image.put(0, columns_of(old, L))
    g, cold = ka.Group(ctx, k, nh, L, 600), ka.Group(ctx, k, nh, L, 600)
    try:
        assert g.add_columns(host, 40) == 0
        if when == "after finalize":
            g.finalize()
            before = check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [3, 39])
            assert not any(q == 2 for q, _, _ in before[1.0])          # nobody holds the new sample yet
        first = g.insert_filters(fresh)
        assert first == 128
        if when == "before finalize":
            g.finalize()
        image.put(first, columns_of(fresh, L))
        assert cold.add_columns(host, 40) == 0 and cold.add_columns(np.ascontiguousarray(image.packed()[:, 16:]), 1) == 128
        cold.finalize()
        after = check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [3, 39, first], twin=cold)
        assert (2, first, len(oracle.unique_kmers(queries[2], k))) in after[1.0]
        if when == "after finalize":
            for t in (1.0, 0.8):      # the old columns' records are what they were
                assert [h for h in after[t] if h[1] < 40] == before[t]
    finally:
        g.close()
        cold.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. across the row widths of the kernel table
# ------------------------------------------------------------------------------------------------------------------

def test_across_the_row_widths_of_the_kernel_table(ka, ctx, oracle):
    """A group of capacity 8192 columns (rows 1 KiB apart): 4000 file columns (500 bytes of a row in use), 200 inserted
    (more than 512), then inserts up to the full KiB.  engine.hip chooses the gather kernel from the row STRIDE, not from
    the bytes in use, so the table gives one and the same kernel at all three widths -- the several-queries-per-wave form
    is for groups whose STRIDE is at most 512 bytes; with early exit a stride of a KiB runs screen + refine throughout."""
    k, nh, L = 15, 2, 10
    rng = np.random.default_rng(6)
    genomes = [random_dna(rng, 60) for _ in range(6)]
    file_cols = rng.random((1 << L, 4000)) < 0.5
    for j, c in enumerate((0, 1999, 3999)):
        file_cols[:, c] |= columns_of(oracle.bloom_bits_from_sequences([genomes[j]], k, nh, L)[None, :], L)[:, 0]
    image = Image(L)
    image.put(0, file_cols)
    queries = [random_dna(rng, 16) for _ in range(58)] + [gn[5:45] for gn in genomes]
    g = ka.Group(ctx, k, nh, L, 8192)
    try:
        assert g.row_stride == 1024
        assert g.add_columns(image.packed(), 4000) == 0
        g.finalize()
        b = ka.Batch(ctx, queries)
        names = []

        def searched():
            got = []
            for flags in (0, ka.SEARCH_EARLY_EXIT):
                r = g.search(b, 1.0, flags)
                assert [tuple(h) for h in r.hits.tolist()] == oracle_hits(oracle, image, k, nh, L, queries, 1.0), (g.row_bytes, flags)
                got.append(r.search_kernel)
            r = g.search(b, 0.8, 0)
            assert [tuple(h) for h in r.hits.tolist()] == oracle_hits(oracle, image, k, nh, L, queries, 0.8), g.row_bytes
            got.append(r.search_kernel)
            names.append(got)
        try:
            assert g.row_bytes == 500
            searched()
            f1 = random_filters(rng, L, 200)
            f1[0] |= oracle.bloom_bits_from_sequences([genomes[3]], k, nh, L)
            first = g.insert_filters(f1)
            assert first == 4096 and g.row_bytes == 537
            image.put(first, columns_of(f1, L))
            searched()
            f2 = random_filters(rng, L, 8192 - 4296)
            f2[0] |= oracle.bloom_bits_from_sequences([genomes[4]], k, nh, L)
            f2[-1] |= oracle.bloom_bits_from_sequences([genomes[5]], k, nh, L)
            assert g.insert_filters(f2) == 4296 and g.row_bytes == 1024 == g.row_stride          # the group is full to the last column
            image.put(4296, columns_of(f2, L))
            searched()
            check_rows(g, image)
        finally:
            b.close()
        assert names[0] == names[1] == names[2], names
        assert names[0][0].startswith("and_kernel<1,8,nt>") and names[0][1].startswith("and_screen_kernel<1,8>") and names[0][2].startswith("count_"), names[0]
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals write nothing
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(ka, ctx, oracle, tmp_path):
    import torch
    from kwage_amd.native import lib
    k, nh, L = 15, 2, 9
    nrows = 1 << L
    rng = np.random.default_rng(7)
    base = random_filters(rng, L, 1000)
    g = ka.Group(ctx, k, nh, L, 1024)                     # stride 128: capacity 1024 columns exactly
    sparse = ka.Group.sparse(ctx, k, nh, L, 1024, np.arange(0, nrows, 2))
    try:
        assert g.insert_filters(base) == 0
        g.finalize()
        image = Image(L)
        image.put(0, columns_of(base, L))
        before = state_of(g, nrows)
        first, ms = C.c_uint64(4242), C.c_float(0)
        extra = random_filters(rng, L, 25)
        dev = torch.from_numpy(np.concatenate([extra, extra], axis=1)).to(torch.device("cuda", ctx.device))

        def refused(rc, want=ERR_ARG):
            assert rc == want, (rc, lib().kwage_last_error())
            assert first.value == 4242 and same_state(state_of(g, nrows), before)

        ins = lib().kwage_group_insert_filters
        refused(ins(g._h, extra.ctypes.data, extra.strides[0], 25, 0, C.byref(first), C.byref(ms)))               # capacity exceeded by one column
        assert b"capacity" in lib().kwage_last_error()
        refused(ins(g._h, extra.ctypes.data, extra.strides[0], 0, 0, C.byref(first), C.byref(ms)))                # n == 0
        refused(ins(g._h, None, extra.strides[0], 5, 0, C.byref(first), C.byref(ms)))                             # NULL arguments
        refused(ins(g._h, extra.ctypes.data, extra.strides[0], 5, 0, None, C.byref(ms)))
        refused(ins(None, extra.ctypes.data, extra.strides[0], 5, 0, C.byref(first), C.byref(ms)))
        refused(ins(g._h, extra.ctypes.data, extra.strides[0] - 1, 5, 0, C.byref(first), C.byref(ms)))            # a stride smaller than a filter
        insd = lib().kwage_group_insert_filters_device
        refused(insd(g._h, dev.data_ptr() + 2, dev.stride(0), 5, 0, C.byref(first), C.byref(ms)))                 # a misaligned device pointer
        refused(insd(g._h, dev.data_ptr(), dev.stride(0) + 2, 5, 0, C.byref(first), C.byref(ms)))                 # ... stride
        refused(insd(g._h, dev.data_ptr(), dev.stride(0), 25, 0, C.byref(first), C.byref(ms)))
        # a sparse group
        sp_before = (sparse.column_span, sparse.num_columns)
        assert ins(sparse._h, extra.ctypes.data, extra.strides[0], 5, 0, C.byref(first), C.byref(ms)) == ERR_ARG and first.value == 4242
        assert b"sparse" in lib().kwage_last_error() and (sparse.column_span, sparse.num_columns) == sp_before
        # `.bloom` files: another num_hash, a flipped payload bit -- each as the LAST of three files
        good = []
        for i in range(3):
            p = str(tmp_path / ("g%d.bloom" % i))
            oracle.write_bloom(p, k, L, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (100 + i))), extra[i])
            good.append(p)
        other = str(tmp_path / "other_hash.bloom")
        oracle.write_bloom(other, k, L, nh + 1, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR200")), extra[4])
        flipped = str(tmp_path / "flipped.bloom")
        raw = bytearray(open(good[0], "rb").read())
        raw[-7] ^= 0x20
        open(flipped, "wb").write(bytes(raw))
        insb = lib().kwage_group_insert_bloom_files
        for bad, want in ((other, ERR_ARG), (flipped, -4), (str(tmp_path / "missing.bloom"), -3)):
            arr = (C.c_char_p * 3)(good[1].encode(), good[2].encode(), bad.encode())
            refused(insb(g._h, arr, 3, 0, C.byref(first), C.byref(ms)), want)
        # between submit and collect: insert and retire are refused, and the search still answers for the group as it was
        queries = [random_dna(rng, 16) for _ in range(20)]
        b = ka.Batch(ctx, queries)
        try:
            pending = g.submit(b, 1.0)
            cols = np.array([5], dtype=np.uint64)
            rc1 = ins(g._h, extra.ctypes.data, extra.strides[0], 5, 0, C.byref(first), C.byref(ms))
            rc2 = lib().kwage_group_retire_columns(g._h, cols.ctypes.data, 1)
            rc3 = insd(g._h, dev.data_ptr(), dev.stride(0), 5, 0, C.byref(first), C.byref(ms))
            r = pending.collect()
            assert (rc1, rc2, rc3) == (ERR_STATE, ERR_STATE, ERR_STATE) and first.value == 4242
            assert [tuple(h) for h in r.hits.tolist()] == oracle_hits(oracle, image, k, nh, L, queries, 1.0)
            assert same_state(state_of(g, nrows), before)
        finally:
            b.close()
        # and the group still takes what fits: 24 columns fill it to the last one
        assert g.insert_filters(extra[:24]) == 1000
        image.put(1000, columns_of(extra[:24], L))
        check_rows(g, image)
    finally:
        g.close()
        sparse.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. retire
# ------------------------------------------------------------------------------------------------------------------

def test_retire(ka, ctx, oracle):
    from kwage_amd.native import lib
    k, nh, L = 15, 2, 8
    rng = np.random.default_rng(8)
    queries = [random_dna(rng, 16) for _ in range(14)] + [random_dna(rng, 40)]
    file_cols = rng.random((1 << L, 21)) < 0.6
    filters = random_filters(rng, L, 30)
    image = Image(L)
    image.put(0, file_cols)
    g = ka.Group(ctx, k, nh, L, 600)
    try:
        assert g.add_columns(image.packed(), 21) == 0
        g.finalize()
        first = g.insert_filters(filters)
        image.put(first, columns_of(filters, L))
        check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [9, 10, first + 2, first + 5])
        # two columns of one byte of the file block, two of one byte of the insert (one column named twice)
        gone = [9, 10, first + 2, first + 5, 9]
        g.retire_columns(gone)
        for c in set(gone):
            image.retire(c)
        check_rows(g, image)                                       # zero where they were, every neighbour unchanged
        assert g.num_columns == 51 - 4
        check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [8, 11, first + 3])
        # again: pad columns now
        before = state_of(g, 1 << L)
        for cols in ([9], [first + 5], [0, first + 2], [g.column_span], [30]):
            arr = np.array(cols, dtype=np.uint64)
            assert lib().kwage_group_retire_columns(g._h, arr.ctypes.data, arr.size) == ERR_ARG
            assert same_state(state_of(g, 1 << L), before)
        # the tail is where it was
        more = random_filters(rng, L, 3)
        assert g.insert_filters(more) == first + 30
        image.put(first + 30, columns_of(more, L))
        check_rows(g, image)
        check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [first + 30])
    finally:
        g.close()
    # a sparse group: over its listed rows
    rows = np.sort(rng.choice(1 << L, size=77, replace=False)).astype(np.uint32)
    sp = ka.Group.sparse(ctx, k, nh, L, 600, rows)
    try:
        img = np.ascontiguousarray(np.packbits(file_cols, axis=1, bitorder="little")[rows])
        assert sp.add_columns(img, 21) == 0
        sp.retire_columns([0, 7, 20])
        want = file_cols[rows].copy()
        want[:, [0, 7, 20]] = False
        assert np.array_equal(sp.read_rows(np.arange(77)), np.packbits(want, axis=1, bitorder="little")) and sp.num_columns == 18
    finally:
        sp.close()


# ------------------------------------------------------------------------------------------------------------------
# 9. FileDatabase
# ------------------------------------------------------------------------------------------------------------------

def test_file_database_add_and_retire_sample(ka, ctx):
    dbs = [os.path.join(GOLDEN, "multi", "dbs")]
    rng = np.random.default_rng(9)
    seq = random_dna(rng, 400)
    query = seq[37:237]
    plain = ka.FileDatabase(ctx, dbs)
    try:
        spans = [(g.column_span, g.num_columns, g.row_stride) for g in plain.groups]
        base_scores, base_acc = plain.score_matrix([query])
        base_hits = plain.search_sequences([query])
    finally:
        plain.close()
    again = ka.FileDatabase(ctx, dbs, headroom=0)
    try:
        assert [(g.column_span, g.num_columns, g.row_stride) for g in again.groups] == spans          # headroom = 0: exactly as before
    finally:
        again.close()
    db = ka.FileDatabase(ctx, dbs, headroom=64)
    try:
        assert [(g.column_span, g.num_columns) for g in db.groups] == [s[:2] for s in spans]
        assert "SRR9999999" not in base_acc and not any(h.accession == "SRR9999999" for h in base_hits)
        gi, col = db.add_sample("SRR9999999", [seq])
        assert gi == 0 and col == (spans[0][0] // 8 + 15) // 16 * 128
        kk = db.groups[0].params.kmer_len
        n_kmers = len(query) - kk + 1
        hits = [h for h in db.search_sequences([query]) if h.accession == "SRR9999999"]
        assert len(hits) == 1 and hits[0].path == "live" and hits[0].column == 0 and hits[0].num_kmers_found == hits[0].num_query_kmer <= n_kmers
        top = db.search_sequences_top([query], 3)
        assert any(h.accession == "SRR9999999" and h.num_kmers_found == h.num_query_kmer for h in top)
        scores, acc = db.score_matrix([query])
        assert acc == base_acc + ["SRR9999999"] and np.array_equal(scores[:, :-1], base_scores) and scores[0, -1] == hits[0].num_query_kmer
        present, acc2 = db.presence_matrix([query], 1.0)
        assert acc2 == acc and present[0, -1]
        near = db.similar_samples(["SRR9999999"], 1)
        assert near[0][0] == "SRR9999999" and near[0][1][0][0] == "SRR9999999" and near[0][1][0][6] == 1.0
        assert db.retire_sample("SRR9999999") == (gi, col)
        assert [h for h in db.search_sequences([query])] == base_hits
        scores, acc = db.score_matrix([query])
        assert acc == base_acc and np.array_equal(scores, base_scores)
        assert db.presence_matrix([query], 1.0)[1] == base_acc
        with pytest.raises(KeyError):
            db.retire_sample("SRR9999999")
        # a sample of a file can go too, and a new one comes in behind the first
        victim = base_acc[0]
        db.retire_sample(victim)
        assert db.score_matrix([query])[1] == base_acc[1:]
        assert db.add_sample("SRR9999998", [seq])[1] == col + 1
        assert db.score_matrix([query])[1] == base_acc[1:] + ["SRR9999998"]
    finally:
        db.close()
