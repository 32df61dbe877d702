"""The overlap matrix (include/kwage_amd.h: kwage_group_column_overlaps; Group.column_overlaps, FileDatabase.sample_overlaps,
`kwage_pairs`): the shared set bits of every pair of listed columns of two RESIDENT groups, an integer matrix product on
the matrix cores.

The expected cells are the model's (tests/overlap_model.py: numpy, none of the planners) over the expected matrices of
tests/group_model.py, never the code under test; on finalized groups also the filter search's
(search_filter_scores(FilterSet.from_columns(...))).  Every case compares the whole block of cells, the sentinel cells
between a row's cells and row_elems included.  Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import group_model as gm
import overlap_model as om
from union_model import _random_image

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
K, NH = om.K, om.NH
PAD = 3                        # sentinel cells behind every row


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


class Pair:
    """A device group and its model, built by the same steps."""

    def __init__(self, ka, ctx, L, capacity):
        self.g = ka.Group(ctx, K, NH, L, capacity)
        self.m = gm.GroupModel(L, gm.stride_of(capacity))
        assert self.g.row_stride == self.m.stride

    def add_columns(self, image, nf):
        assert self.g.add_columns(image, nf) == self.m.add_columns(image, nf)

    def insert(self, filters):
        assert self.g.insert_filters(filters) == self.m.insert(filters)

    def retire(self, cols):
        self.g.retire_columns(cols)
        assert self.m.retire(cols) == 0

    def set_bits(self, rows, cols):
        self.g.set_bits(np.asarray(rows), np.asarray(cols))
        assert self.m.set_bits(rows, cols) == 0

    def finalize(self):
        self.g.finalize()
        self.m.finalize()

    def close(self):
        self.g.close()


def check(ka, a, cols_a, b=None, cols_b=None, same_as_a=False):
    """One call against the model (b None: the symmetric form; same_as_a: b is a's own group), whole block; a finalized
    b also against the filter search.  Returns (cells, stats)."""
    import torch
    other = a if same_as_a else b
    want = om.of_models(a.m, cols_a, other.m if other else None, cols_b)
    n_a, n_b = want.shape
    out = torch.full((n_a, n_b + PAD), om.SENTINEL, dtype=torch.int32, device="cuda")
    got, st = a.g.column_overlaps(cols_a, other.g if other else None, cols_b, out=out, timing=True)
    cells = got.cpu().numpy().view(np.uint32)
    assert np.array_equal(cells[:, :n_b], want), (np.argwhere(cells[:, :n_b] != want)[:5], st)
    assert (cells[:, n_b:] == np.uint32(om.SENTINEL & 0xFFFFFFFF)).all()
    symmetric = other is None
    sa, ga_ = om.blocks_of(cols_a, a.m.span)
    sb, gb_ = (0, 0) if symmetric else om.blocks_of(cols_b, other.m.span)
    assert (st["n_a"], st["n_b"], st["rows"], st["symmetric"]) == (n_a, n_b, a.m.nrows, int(symmetric)), st
    assert (st["straight_blocks"], st["gathered_blocks"], st["tiles"]) == (sa + sb, ga_ + gb_, om.tiles_of(n_a, n_b, symmetric)), st
    assert st["kernel"] == ("" if not st["tiles"] else "overlap_mfma_kernel" if st["splits"] == 1 else "overlap_mfma_kernel+overlap_combine_kernel"), st
    assert (st["kernel_ms"] > 0) == (st["tiles"] > 0)
    # the host form: the same cells
    host, _ = a.g.column_overlaps_host(cols_a, other.g if other else None, cols_b)
    assert host.dtype == np.uint32 and np.array_equal(host, want)
    # the filter search's answer, where it can be had (a filter set takes live columns, each once)
    tgt = other or a
    fa = np.flatnonzero(a.m.real) if cols_a is None else np.asarray(cols_a)
    if tgt.m.finalized and a.m.finalized and n_a and n_b and len(set(fa.tolist())) == len(fa):
        fs = ka.FilterSet.from_columns(a.g, fa)
        try:
            scores = ka.search_filter_scores(tgt.g, fs).scores
        finally:
            fs.close()
        side_b = cols_a if symmetric else cols_b
        tb = np.arange(tgt.m.span) if side_b is None else np.asarray(side_b)
        assert np.array_equal(scores[:, tb], want[fa] if cols_a is None else want)
    return cells[:, :n_b], st


@pytest.fixture(scope="module")
def world(ka, ctx):
    """Two open groups of 1024 rows with different strides: A holds a file block with garbage in its pad bits, live
    inserts, retired columns with bits planted in them; B an open tail."""
    rng = np.random.default_rng(2026)
    L = 10
    a, b = Pair(ka, ctx, L, 1000), Pair(ka, ctx, L, 3000)
    a.add_columns(_random_image(rng, 1 << L, 77), 77)           # columns 0 .. 76, 77 .. 79 garbage, then pad to 128
    a.insert(gm.random_filters(rng, L, 333))                    # 128 .. 460
    a.retire([130, 200, 201, 300])
    a.set_bits([1, 5, 900, 5, 6], [130, 130, 200, 78, 100])     # bits in retired and pad columns beside listed ones
    b.insert(gm.random_filters(rng, L, 310))
    b.retire([33])
    b.set_bits([0, 1, 2], [33, 33, 33])
    yield a, b, rng
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------
# rows: fewer than one group of 32, exactly one, several steps; the parts
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", om.ROW_LOGS)
def test_rows(ka, ctx, L):
    rng = np.random.default_rng(100 + L)
    a, b = Pair(ka, ctx, L, 400), Pair(ka, ctx, L, 1400)
    try:
        a.insert(gm.random_filters(rng, L, 70))
        b.insert(gm.random_filters(rng, L, 45))
        check(ka, a, None)
        check(ka, a, rng.permutation(70)[:33], b, None)
        a.finalize()
        b.finalize()
        check(ka, a, rng.permutation(70)[:40], b, np.arange(32, 45))
    finally:
        a.close()
        b.close()


def test_every_split_count_gives_the_same_cells(ka, ctx, world):
    a, b, rng = world
    la, lb = om.list_of(rng, "shuffle", a.m.real, 129), om.list_of(rng, "mixed", b.m.real)
    seen = []
    for splits in om.SPLITS:
        with ctx.tuning(overlap_splits=splits):
            cells, st = check(ka, a, la, b, lb)
            sym, st2 = check(ka, a, None)
        assert st["splits"] == st2["splits"] == (splits or 1)
        seen.append((cells, sym))
    for cells, sym in seen[1:]:
        assert np.array_equal(cells, seen[0][0]) and np.array_equal(sym, seen[0][1])


# ------------------------------------------------------------------------------------------------------------------
# columns: the counts around a block and a tile on either side, n_a != n_b the rule
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", om.COUNTS)
def test_counts_on_either_side(ka, world, n):
    a, b, rng = world
    check(ka, a, om.list_of(rng, "shuffle", a.m.real, n), b, om.list_of(rng, "reversed", b.m.real, 40))
    check(ka, b, om.list_of(rng, "reversed", b.m.real, 40), a, om.list_of(rng, "shuffle", a.m.real, n))
    check(ka, a, om.list_of(rng, "shuffle", a.m.real, n))


@pytest.mark.parametrize("n_b", om.PAIR_COUNTS)
@pytest.mark.parametrize("n_a", om.PAIR_COUNTS)
def test_count_pairs(ka, world, n_a, n_b):
    a, b, rng = world
    check(ka, a, np.flatnonzero(a.m.real)[:n_a], b, om.list_of(rng, "shuffle", b.m.real, n_b))


@pytest.mark.parametrize("kind", om.LIST_KINDS)
def test_lists(ka, world, kind):
    a, b, rng = world
    cols = om.list_of(rng, kind, a.m.real)
    check(ka, a, cols)
    check(ka, a, cols, b, None)
    check(ka, b, None, a, cols)
    check(ka, a, cols, same_as_a=True, cols_b=om.list_of(rng, "shuffle", a.m.real, 33))


def test_null_lists_with_dead_columns(ka, world):
    a, b, rng = world
    cells, st = check(ka, a, None, b, None)
    assert st["gathered_blocks"] == 0 and not cells[[78, 100, 130, 200]].any() and not cells[:, 33].any()
    sym, _ = check(ka, a, None)
    assert not sym[130].any() and not sym[:, 78].any() and sym[129, 129] > 0
    assert np.array_equal(check(ka, a, None, same_as_a=True)[0], sym)


# ------------------------------------------------------------------------------------------------------------------
# the symmetric form
# ------------------------------------------------------------------------------------------------------------------

def test_symmetric_form(ka, ctx):
    rng = np.random.default_rng(5)
    L = 10
    a = Pair(ka, ctx, L, 1000)
    try:
        a.insert(gm.random_filters(rng, L, 300))
        a.retire([7, 140])
        a.finalize()
        for cols in (None, om.list_of(rng, "shuffle", a.m.real, 300)[:290], np.arange(160, 288)):
            sym, st = check(ka, a, cols)
            axa, st2 = check(ka, a, cols, same_as_a=True, cols_b=cols)
            assert np.array_equal(sym, axa) and np.array_equal(sym, sym.T)
            n = len(sym)
            t = (n + 127) // 128
            assert st["symmetric"] == 1 and st["tiles"] == t * (t + 1) // 2 and st2["symmetric"] == 0 and st2["tiles"] == t * t
            bits = a.g.column_bits()
            assert np.array_equal(np.diag(sym), bits if cols is None else bits[cols])
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------------
# groups
# ------------------------------------------------------------------------------------------------------------------

def test_a_span_across_column_8192(ka, ctx):
    rng = np.random.default_rng(8192)
    L = 5
    a, b = Pair(ka, ctx, L, 8500), Pair(ka, ctx, L, 300)
    try:
        a.add_columns(_random_image(rng, 1 << L, 8100), 8100)
        a.insert(gm.random_filters(rng, L, 200))                # 8192 .. 8391
        b.insert(gm.random_filters(rng, L, 33))
        assert a.m.span == 8392
        across = np.concatenate([np.arange(8000, 8100), np.arange(8192, 8392)])
        check(ka, a, across)
        check(ka, a, list(range(8064, 8100)) + list(range(8192, 8256)), b, None)
        cells, st = check(ka, b, None, a, None)                 # every column of a wide group, the pad around 8100 .. 8191 inside
        assert st["tiles"] == 66 and not cells[:, 8100:8192].any() and cells[:, 8192:].any()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n", [1, 33, 129])
def test_an_open_tail(ka, ctx, n):
    rng = np.random.default_rng(n)
    L = 6
    a = Pair(ka, ctx, L, 600)
    try:
        a.insert(gm.random_filters(rng, L, n))
        assert a.m.span == (n + 7) // 8 * 8
        check(ka, a, None)
        check(ka, a, [n - 1], same_as_a=True, cols_b=None)
        a.finalize()
        check(ka, a, None)
    finally:
        a.close()


def test_a_group_emptied_by_a_compaction(ka, ctx):
    import torch
    rng = np.random.default_rng(9)
    L = 6
    a, b = Pair(ka, ctx, L, 600), Pair(ka, ctx, L, 600)
    try:
        a.insert(gm.random_filters(rng, L, 5))
        b.insert(gm.random_filters(rng, L, 5))
        a.retire([0, 1, 2, 3, 4])
        a.g.compact()
        a.m.compact()
        assert a.g.column_span == a.m.span == 0
        out = torch.full((8, 12), om.SENTINEL, dtype=torch.int32, device="cuda")
        for other in (None, a.g, b.g):
            got, st = a.g.column_overlaps(None, other, None, out=out[:0])
            assert (st["n_a"], st["tiles"], st["kernel"]) == (0, 0, "")
        got, st = b.g.column_overlaps(None, a.g, None, out=out[:, :0])
        assert (st["n_a"], st["n_b"], st["tiles"]) == (8, 0, 0) and (out.cpu().numpy() == om.SENTINEL).all()
        assert a.g.column_overlaps_host()[0].shape == (0, 0)
        a.insert(gm.random_filters(rng, L, 3))                  # and it lives on
        check(ka, a, None, b, None)
    finally:
        a.close()
        b.close()


def test_a_fold(ka, ctx, world):
    a, b, rng = world
    fa, _ = a.g.fold(7)
    fb, _ = b.g.fold(7)
    try:
        pa, pb = Pair.__new__(Pair), Pair.__new__(Pair)
        pa.g, pa.m = fa, a.m.fold(7)[0]
        pb.g, pb.m = fb, b.m.fold(7)[0]
        check(ka, pa, om.list_of(rng, "mixed", a.m.real), pb, None)
        check(ka, pa, None)
    finally:
        fa.close()
        fb.close()


def test_finalized_groups_against_the_filter_search(ka, ctx, world):
    a, b, rng = world
    ta, tb = Pair(ka, ctx, 10, 1000), Pair(ka, ctx, 10, 3000)
    try:
        for src, dst in ((a, ta), (b, tb)):
            real = np.flatnonzero(src.m.real)
            dst.insert(src.g.export_filters(real))
            dst.retire([3, 64])
            dst.finalize()
        check(ka, ta, om.list_of(rng, "shuffle", ta.m.real, 129), tb, om.list_of(rng, "mixed", tb.m.real))
        check(ka, ta, None, tb, None)
        check(ka, ta, None)
        check(ka, ta, om.list_of(rng, "repeat", ta.m.real), tb, om.list_of(rng, "shifted", tb.m.real))
    finally:
        ta.close()
        tb.close()


# ------------------------------------------------------------------------------------------------------------------
# planted data: what a transposed or mirrored tile cannot pass
# ------------------------------------------------------------------------------------------------------------------

def test_planted_columns(ka, ctx):
    L = 14
    rows = 1 << L
    r = np.arange(rows)
    a, b = Pair(ka, ctx, L, 400), Pair(ka, ctx, L, 1400)
    try:
        n_a, n_b = 129, 40
        ca = np.zeros((rows, n_a), dtype=bool)
        for i in range(n_a):
            ca[:, i] = r < 100 * (i + 1)                        # nested: column i holds the first 100 (i + 1) rows
        ca[:, 7] = True                                         # one full column
        ca[:, 8] = False                                        # one empty column
        cb = np.zeros((rows, n_b), dtype=bool)
        for j in range(n_b):
            cb[:, j] = (r >> (j % 14)) & 1 == 1                 # every column of b half full
        cb[:, 5] = True                                         # the all-ones pair with a's column 7
        cb[:, 6] = False
        a.insert(gm.filters_of(ca))
        b.insert(gm.filters_of(cb))
        cells, _ = check(ka, a, None, b, None)
        assert cells[7, 5] == rows and (cells[7, :n_b] == cb.sum(axis=0)).all() and not cells[8].any() and not cells[:, 6].any()
        assert cells[0, 0] == 50 and cells[1, 0] == 100 and cells[0, 1] == 50 and cells[3, 1] == 200
        sym, _ = check(ka, a, None)
        i, j = 20, 90
        assert sym[i, j] == sym[j, i] == 100 * (i + 1) and sym[7, 7] == rows
        # nested against nested, n_a != n_b: cell (i, j) = 100 (min(i, j) + 1), and (i, j) != (j, i) in what is listed
        la, lb = np.arange(10, 43), np.arange(60, 129)
        axb, _ = check(ka, a, la, same_as_a=True, cols_b=lb)
        assert axb.shape == (33, 69) and (axb == (100 * (la + 1))[:, None]).all()
        bxa, _ = check(ka, a, lb, same_as_a=True, cols_b=la)
        assert np.array_equal(bxa, axb.T) and not np.array_equal(bxa[:33, :33], axb[:33, :33])
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------
# refusals: in order, each found before a kernel runs or a byte is allocated
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_in_order_leave_the_outputs_alone(ka, ctx, world):
    import torch
    from kwage_amd import native
    lib = native.lib()
    a, b, rng = world
    L = 10
    sparse = ka.Group.sparse(ctx, K, NH, L, 1024, np.arange(0, 1 << L, 2))
    differing = [ka.Group(ctx, K - 10, NH, L, 256), ka.Group(ctx, K, NH + 1, L, 256), ka.Group(ctx, K, NH, L - 1, 256)]
    searched = ka.Group(ctx, K, NH, L, 256)
    other_ctx = ka.Context(0)
    foreign = ka.Group(other_ctx, K, NH, L, 256)
    batch = ka.Batch(ctx, [gm.random_dna(rng, 40) for _ in range(8)])
    try:
        for g in differing + [searched, foreign]:
            g.insert_filters(gm.random_filters(rng, int(g.params.log_2_filter_len), 5))
        searched.finalize()
        searched.submit(batch, 1.0).collect()
        ctx.sync()
        out = torch.full((8, 8), om.SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        free = ctx.mem_info()[0]
        good = (C.c_uint64 * 3)(0, 1, 2)
        beyond = (C.c_uint64 * 3)(0, 100000, 130)               # (the later faults every earlier refusal carries)

        def call(ga, ca, na, gb, cb, nb, row_elems, cells=True):
            st = native.OverlapStats(n_a=77, tiles=77, kernel_ms=-1.0)
            rc = lib.kwage_group_column_overlaps_device(ga, ca, na, gb, cb, nb, out.data_ptr() if cells else None, row_elems, 2, C.byref(st))
            assert (st.n_a, st.tiles, st.kernel_ms) == (77, 77, -1.0)
            return rc, lib.kwage_last_error()

        def refused(got, status, word):
            assert got[0] == status and word in got[1], (got, word)

        A, B = a.g._h, b.g._h
        refused(call(None, beyond, 3, foreign._h, beyond, 0, 0), ERR_ARG, b"NULL a")
        refused(call(A, beyond, 0, foreign._h, beyond, 0, 0, cells=False), ERR_ARG, b"NULL cells")
        refused(call(A, None, 3, foreign._h, beyond, 0, 0), ERR_ARG, b"NULL cols_a with n_a = 3")
        refused(call(A, beyond, 0, foreign._h, beyond, 0, 0), ERR_ARG, b"n_a is 0")
        refused(call(A, beyond, 3, foreign._h, None, 3, 0), ERR_ARG, b"NULL cols_b with n_b = 3")
        refused(call(A, beyond, 3, foreign._h, beyond, 0, 0), ERR_ARG, b"n_b is 0")
        refused(call(A, beyond, 3, None, beyond, 3, 0), ERR_ARG, b"cols_b without b")
        refused(call(A, beyond, 3, foreign._h, beyond, 3, 0), ERR_ARG, b"different contexts")
        refused(call(A, beyond, 3, sparse._h, beyond, 3, 0), ERR_ARG, b"sparse")
        refused(call(sparse._h, beyond, 3, A, beyond, 3, 0), ERR_ARG, b"sparse")
        refused(call(sparse._h, beyond, 3, None, None, 0, 0), ERR_ARG, b"sparse")
        for g, word in zip(differing, (b"kmer_len", b"num_hash", b"log_2_filter_len")):
            refused(call(A, beyond, 3, g._h, beyond, 3, 0), ERR_ARG, word)
            refused(call(g._h, beyond, 3, A, beyond, 3, 0), ERR_ARG, word)
        # (hash_func and L = 32: kwage_group_create makes no such pair of groups here -- tests/sanitize/overlap_sanitize.cpp's)
        pending = searched.submit(batch, 1.0)
        got = [call(A, beyond, 3, B, beyond, 3, 2), call(A, beyond, 3, B, None, 0, b.g.column_span - 1), call(A, None, 0, None, None, 0, a.g.column_span - 1),
               call(A, beyond, 3, B, beyond, 3, 3), call(A, beyond, 3, None, None, 0, 3)]
        pending.collect()
        ctx.sync()
        for g_ in got[:3]:
            refused(g_, ERR_ARG, b"row_elems")
        refused(got[3], ERR_STATE, b"pending")
        refused(got[4], ERR_STATE, b"pending")
        refused(call(A, beyond, 3, B, beyond, 3, 3), ERR_ARG, b"column 100000 is at or beyond the span %d" % a.g.column_span)
        refused(call(A, (C.c_uint64 * 3)(0, 130, 100000), 3, B, beyond, 3, 3), ERR_ARG, b"column 130 is a pad or retired column")
        refused(call(A, (C.c_uint64 * 3)(0, 78, 0), 3, B, beyond, 3, 3), ERR_ARG, b"column 78 is a pad or retired column")
        refused(call(A, good, 3, B, beyond, 3, 3), ERR_ARG, b"column 100000 is at or beyond the span %d" % b.g.column_span)
        refused(call(A, good, 3, B, (C.c_uint64 * 3)(0, 33, 100000), 3, 3), ERR_ARG, b"column 33 is a pad or retired column")
        refused(call(A, beyond, 3, None, None, 0, 3), ERR_ARG, b"column 100000")
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == om.SENTINEL).all() and ctx.mem_info()[0] == free
        # and the same call succeeds afterwards, a column listed twice, without stats too
        assert lib.kwage_group_column_overlaps_device(A, (C.c_uint64 * 3)(0, 1, 0), 3, B, good, 3, out.data_ptr(), 8, 0, None) == 0
        want = om.of_models(a.m, [0, 1, 0], b.m, [0, 1, 2])
        cells = out.cpu().numpy()
        assert np.array_equal(cells[:3, :3].view(np.uint32), want) and (cells[3:] == om.SENTINEL).all() and (cells[:, 3:] == om.SENTINEL).all()
    finally:
        batch.close()
        for g in [sparse, searched, foreign] + differing:
            g.close()
        other_ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# FileDatabase.sample_overlaps and kwage_pairs, on the golden `.db` files
# ------------------------------------------------------------------------------------------------------------------

def db_columns(oracle, path):
    """([run accession of column j], bool [2^L, num_filter]) of a `.db` file, read with the oracle's reader."""
    f = oracle.read_db(path)
    bits = np.unpackbits(np.asarray(f.rows), axis=1, bitorder="little")[:, :f.header.num_filter].astype(bool)
    return [oracle.accession_to_str(f.info(j).run_accession) for j in range(f.header.num_filter)], bits, f


def golden_files(root):
    out = []
    for d, _, names in os.walk(root):
        out.extend(os.path.join(d, n) for n in names if n.endswith(".db"))
    return sorted(out)


def expected_pairs(oracle, files, accessions=None):
    """(accessions, int64 shared matrix) over the samples of `files` that share the first chosen sample's parameters."""
    cols = []
    for f in files:
        accs, bits, h = db_columns(oracle, f)
        key = (h.header.kmer_len, h.header.num_hash, h.header.log_2_filter_len, h.header.hash_func)
        cols.extend((acc, key, bits[:, j]) for j, acc in enumerate(accs))
    if accessions is not None:
        first = {}
        for c in cols:
            first.setdefault(c[0], c)
        cols = [first[a] for a in accessions]
    left_out = [c[0] for c in cols if c[1] != cols[0][1]]
    cols = [c for c in cols if c[1] == cols[0][1]]
    m = np.stack([c[2] for c in cols], axis=1).astype(np.int64)
    return [c[0] for c in cols], m.T @ m, left_out


def jaccard_of(shared):
    bits = np.diag(shared)
    union = bits[:, None] + bits[None, :] - shared
    return np.where(union > 0, shared.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)


def test_sample_overlaps_on_the_golden_files(ka, ctx, oracle, golden_dir):
    import warnings
    root = os.path.join(golden_dir, "basic", "db")
    db = ka.FileDatabase(ctx, [root])
    try:
        order = [db._accession(path, c) for _, _, path, c in db._samples()]
        names, want, _ = expected_pairs(oracle, db.files)
        assert sorted(names) == sorted(order)
        got_names, got = db.sample_overlaps()
        at = [names.index(a) for a in got_names]
        assert got_names == order and got.dtype == np.uint32 and np.array_equal(got, want[np.ix_(at, at)])
        pick = [order[5], order[0], order[17], order[5]]
        got_names, jac = db.sample_overlaps(pick, jaccard=True)
        at = [names.index(a) for a in pick]
        assert got_names == pick and jac.dtype == np.float64 and np.array_equal(jac, jaccard_of(want[np.ix_(at, at)]))
        with pytest.raises(KeyError):
            db.sample_overlaps(["SRR0000000"])
    finally:
        db.close()
    # several groups: pairs between the groups of one parameter set, the others left out and named
    db = ka.FileDatabase(ctx, [os.path.join(golden_dir, "multi", "dbs")])
    try:
        assert len(db.groups) >= 2
        order = [db._accession(path, c) for _, _, path, c in db._samples()]
        names, want, left_out = expected_pairs(oracle, db.files, order)
        assert left_out
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got_names, got = db.sample_overlaps()
        assert got_names == names and np.array_equal(got, want)
        assert len(w) == 1 and all(a in str(w[0].message) for a in left_out)
    finally:
        db.close()


@pytest.mark.parametrize("jaccard", [False, True])
def test_kwage_pairs(ka, oracle, golden_dir, tmp_path, jaccard):
    from kwage_amd import native
    tool = os.path.join(os.path.dirname(native.KWAGE_DBTOOL_BIN), "kwage_pairs")
    root = os.path.join(golden_dir, "multi", "dbs")

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    # argument errors end the program before a device is opened
    r = run()
    assert r.returncode == 1 and "Usage for kwage_pairs" in r.stderr
    r = run("-d", root, "-s", "SRR0000000")
    assert r.returncode == 1 and "SRR0000000" in r.stderr and not r.stdout
    r = run("-d", str(tmp_path))
    assert r.returncode == 1 and "Please provide at least one database file" in r.stderr
    # every sample: the files in the program's own order (its header line says it)
    out = str(tmp_path / "pairs.tsv")
    r = run("-d", root, "-o", out, *(["--jaccard"] if jaccard else []))
    assert r.returncode == 0, r.stderr
    lines = open(out).read().splitlines()
    head = lines[0].split("\t")
    assert head[0] == "sample" and len(lines) == len(head)
    # (the program's file order is the directory's: take its header's, and the model by accession)
    all_names, all_want, _ = expected_pairs(oracle, golden_files(root), head[1:])
    assert all_names == head[1:]
    assert r.stderr.count("Skipping ") >= 1
    for i, line in enumerate(lines[1:]):
        cells = line.split("\t")
        assert cells[0] == head[1 + i]
        if jaccard:
            assert cells[1:] == ["%.6f" % v for v in jaccard_of(all_want)[i]]
        else:
            assert [int(c) for c in cells[1:]] == all_want[i].tolist()
    # listed samples, positional and with -s, a repeat among them
    pick = [head[3], head[1], head[3]]
    r = run("-d", root, "-s", pick[0], pick[1], pick[2], *(["--jaccard"] if jaccard else []))
    assert r.returncode == 0, r.stderr
    rows = [x.split("\t") for x in r.stdout.splitlines()]
    assert rows[0] == ["sample"] + pick and [x[0] for x in rows[1:]] == pick
    at = [head[1:].index(a) for a in pick]
    sub = all_want[np.ix_(at, at)]
    if jaccard:
        assert [x[1:] for x in rows[1:]] == [["%.6f" % v for v in row] for row in jaccard_of(sub)]
    else:
        assert [[int(c) for c in x[1:]] for x in rows[1:]] == sub.tolist()
