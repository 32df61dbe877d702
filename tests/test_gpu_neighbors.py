"""Nearest-neighbour lists (include/kwage_amd.h: kwage_group_column_neighbors; Group.column_neighbors,
FileDatabase.sample_neighbors, `kwage_neighbors`): each listed column's k best partners under an exact key, chosen on the
device from the overlap matrix's cells.

The expected lists are the model's (tests/neighbors_model.py: the overlap model's cells, Python integers and Fractions, a
sort) over the expected matrices of tests/group_model.py, never the code under test.  Every comparison is exact equality
of the whole records and counts arrays, for the device form and the host form."""
import ctypes as C
import os
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import group_model as gm
import neighbors_model as nm
import overlap_model as om
from union_model import _random_image

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
K, NH = om.K, om.NH
STRIP_BYTES = 256 << 20
METRICS = (nm.SHARED, nm.JACCARD)


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


def check(a, cols_a, b=None, cols_b=None, k=5, metric=nm.JACCARD, min_shared=0, skip_self=False, same_as_a=False, strip_bytes=STRIP_BYTES, want=None):
    """One call against the model (b None: a's list is also the candidate list; same_as_a: b is a's own group): records
    and counts whole, the device form and the host form.  Returns (records, counts, stats)."""
    other = a if same_as_a else b
    if want is None:
        want = nm.of_models(a.m, cols_a, other.m if other else None, cols_b, k, metric, min_shared, skip_self)
    rec, cnt, st = a.g.column_neighbors(k, cols_a, other.g if other else None, cols_b, metric=metric, min_shared=min_shared, skip_self=skip_self, timing=True)
    rec, cnt = rec.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert rec.shape == want[0].shape and np.array_equal(cnt, want[1]), (cnt[:20], want[1][:20], st)
    assert np.array_equal(rec, want[0]), (np.argwhere(rec != want[0])[:5], st)
    n_a = len(want[1])
    n_b = n_a if other is None else other.m.span if cols_b is None else len(cols_b)
    strips, entries, tiles = nm.stats_of(n_a, n_b, strip_bytes)
    assert (st["n_a"], st["n_b"], st["rows"], st["metric"]) == (n_a, n_b, a.m.nrows, METRICS.index(metric)), st
    assert (st["strips"], st["strip_entries"], st["tiles"], st["records"]) == (strips, entries, tiles if n_b else 0, int(want[1].sum())), st
    assert st["kernel"] in (("",) if not n_a else ("neighbors_select_kernel",) if not n_b else
                            ("overlap_mfma_kernel+neighbors_select_kernel", "overlap_mfma_kernel+overlap_combine_kernel+neighbors_select_kernel")), st
    assert (st["kernel_ms"] > 0) == (n_a > 0)
    hrec, hcnt, hst = a.g.column_neighbors_host(k, cols_a, other.g if other else None, cols_b, metric=metric, min_shared=min_shared, skip_self=skip_self)
    assert hrec.dtype == hcnt.dtype == np.uint32 and np.array_equal(hrec, want[0]) and np.array_equal(hcnt, want[1])
    assert hst["records"] == st["records"] and hst["kernel_ms"] == 0
    return rec, cnt, st


@pytest.fixture(scope="module")
def world(ka, ctx):
    """Two open groups of 1024 rows with different strides: A holds a file block with garbage in its pad bits, live
    inserts, retired columns with bits planted in them; B an open tail (test_gpu_overlap.py's world)."""
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
# rows: at 1 and 32 rows nearly every key ties -- the order is the indices'
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [0, 5, 10])
def test_rows(ka, ctx, L):
    rng = np.random.default_rng(200 + L)
    a, b = Pair(ka, ctx, L, 400), Pair(ka, ctx, L, 1400)
    try:
        a.insert(gm.random_filters(rng, L, 70))
        b.insert(gm.random_filters(rng, L, 45))
        for metric in METRICS:
            for k in (1, 5):
                rec, cnt, _ = check(a, None, b, None, k=k, metric=metric)
                check(a, None, k=k, metric=metric)
                if L < 10:
                    keys = [[nm.key_of(metric, *r[1:]) for r in row[:c]] for row, c in zip(rec.tolist(), cnt)]
                    assert any(len(set(ks)) < len(ks) for ks in keys if len(ks) > 1) or k == 1
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------
# k: all candidates, more than there are, the cap against more candidates than one round of the lanes reads
# ------------------------------------------------------------------------------------------------------------------

def test_k_edges(ka, ctx):
    rng = np.random.default_rng(77)
    L = 5
    a, b, wide = Pair(ka, ctx, L, 400), Pair(ka, ctx, L, 1400), Pair(ka, ctx, L, 1600)
    try:
        a.insert(gm.random_filters(rng, L, 70))
        b.insert(gm.random_filters(rng, L, 45))
        wide.insert(gm.random_filters(rng, L, 1500))
        for metric in METRICS:
            rec, cnt, _ = check(a, None, b, None, k=45, metric=metric)
            assert (cnt[:70] == 45).all()
            rec, cnt, _ = check(a, None, b, None, k=60, metric=metric, min_shared=1)
            assert (cnt < 60).all() and (rec[:, 45:] == nm.FILLER).all()
            rec, cnt, _ = check(a, [3, 69, 3, 0], wide, None, k=1024, metric=metric)
            assert (cnt == 1024).all()
            rec, cnt, _ = check(wide, [0, 1499, 700], same_as_a=True, cols_b=None, k=1024, metric=metric, skip_self=True)
            assert (cnt == 1024).all() and (rec[:, :, 0] != np.array([0, 1499, 700])[:, None]).all()
    finally:
        for p in (a, b, wide):
            p.close()


def test_k_1024_on_the_span_across_column_8192(ka, ctx):
    rng = np.random.default_rng(8192)
    L = 5
    a, b = Pair(ka, ctx, L, 8500), Pair(ka, ctx, L, 300)
    try:
        a.add_columns(_random_image(rng, 1 << L, 8100), 8100)
        a.insert(gm.random_filters(rng, L, 200))                # 8192 .. 8391
        b.insert(gm.random_filters(rng, L, 33))
        assert a.m.span == 8392
        for metric in METRICS:
            rec, cnt, _ = check(b, [0, 32, 7], a, None, k=1024, metric=metric)
            assert (cnt == 1024).all() and not ((rec[:, :, 0] >= 8100) & (rec[:, :, 0] < 8192)).any()
        check(b, [5], a, None, k=1024, metric=nm.SHARED, min_shared=3)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------
# planted keys: what a float key cannot order
# ------------------------------------------------------------------------------------------------------------------

def test_planted_keys(ka, ctx):
    L = 14
    rows = 1 << L
    r = np.arange(rows)
    a = Pair(ka, ctx, L, 400)
    try:
        cols = np.zeros((rows, 50), dtype=bool)
        cols[:, 0] = r < 7500                                   # the query: 7500 bits
        cols[:, 1] = (r < 4999) | ((r >= 7500) & (r < 7500 + 2499))     # shared 4999, own 2499: 4999 / 9999
        cols[:, 2] = (r < 5000) | ((r >= 7500) & (r < 7500 + 2501))     # shared 5000, own 2501: 5000 / 10001, the larger by 1e-8
        cols[:, 3] = cols[:, 0]                                 # identical: s == u
        cols[:, 4] = False                                      # empty: u = bits_a, s = 0
        cols[:, 5] = True                                       # full
        cols[:, 6] = False                                      # a second empty one: against 4, u == 0
        for j in range(7, 47):
            cols[:, j] = (r % 3 == 0) & (r < 9000)              # forty copies of one filter: every key equal
        cols[:, 47:] = np.random.default_rng(14).random((rows, 3)) < 0.3
        a.insert(gm.filters_of(cols))
        # float32 keys would not tell the planted pair apart (or would turn it round)
        f1, f2 = np.float32(5000) / np.float32(10001), np.float32(4999) / np.float32(9999)
        assert Fraction(5000, 10001) > Fraction(4999, 9999) and not f1 > f2
        for skip in (False, True):
            rec, cnt, _ = check(a, None, k=50, metric=nm.JACCARD, skip_self=skip)
            mine = rec[0, :cnt[0]].tolist()
            order = [m[0] for m in mine]
            assert order.index(2) + 1 == order.index(1) and [m[1:] for m in mine if m[0] in (1, 2)] == [[5000, 7500, 7501], [4999, 7500, 7498]]
            assert order[:4] == ([3, 2, 1, 5] if skip else [0, 3, 2, 1]) and rec[4, 0].tolist() == [0, 0, 0, 7500] and rec[4, 6 - int(skip)].tolist() == [6, 0, 0, 0]
            assert rec[5, 0].tolist() == ([2, 7501, rows, 7501] if skip else [5, rows, rows, rows])
            copies = [m[0] for m in rec[7, :cnt[7]].tolist() if 7 <= m[0] < 47]
            assert copies == list(range(8 if skip else 7, 47)) and copies == [m[0] for m in rec[7, :len(copies)].tolist()]
        rec, cnt, _ = check(a, None, k=50, metric=nm.SHARED)
        assert rec[0, 0].tolist() == [0, 7500, 7500, 7500] and rec[0, 1, 0] == 3 and rec[0, 2, 0] == 5
        check(a, [4, 6, 0, 5], same_as_a=True, cols_b=[6, 4, 1, 2, 5, 0, 3], k=7)
        check(a, [0], same_as_a=True, cols_b=[1, 2], k=2)
        check(a, [0], same_as_a=True, cols_b=[2, 1], k=1)
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------------
# skip-self, dead columns, min_shared
# ------------------------------------------------------------------------------------------------------------------

def test_skip_self(ka, world):
    a, b, rng = world
    rep = om.list_of(rng, "repeat", a.m.real)
    for metric in METRICS:
        rec, cnt, _ = check(a, rep, k=6, metric=metric, skip_self=True)
        for i, c in enumerate(rep):
            assert cnt[i] == min(6, int((rep != c).sum())) and not any(rep[j] == c for j in rec[i, :cnt[i], 0])
        plain, _, _ = check(a, rep, k=6, metric=metric)
        assert not np.array_equal(plain, rec)
        listed = om.list_of(rng, "shuffle", a.m.real, 33)
        rec, cnt, _ = check(a, listed, same_as_a=True, cols_b=None, k=4, metric=metric, skip_self=True)
        assert (rec[:, :, 0] != listed[:, None]).all() and (cnt == 4).all()
        # another group: the flag has no effect
        lb = om.list_of(rng, "reversed", b.m.real, 40)
        with_flag, _, _ = check(a, listed, b, lb, k=4, metric=metric, skip_self=True)
        without, _, _ = check(a, listed, b, lb, k=4, metric=metric)
        assert np.array_equal(with_flag, without)


def test_dead_columns(ka, world):
    a, b, rng = world
    for metric in METRICS:
        rec, cnt, _ = check(a, None, b, None, k=7, metric=metric)
        assert not cnt[[78, 100, 130, 200, 201, 300]].any() and (cnt[np.flatnonzero(a.m.real)] == 7).all() and not (rec[:, :, 0] == 33).any()
        rec, cnt, _ = check(a, None, k=3, metric=metric, skip_self=True)
        dead = np.flatnonzero(~a.m.real)
        assert not cnt[dead].any() and (rec[dead] == nm.FILLER).all() and not np.isin(rec[:, :, 0], dead).any()
        check(b, None, a, None, k=460, metric=metric)
    for cols, other, cols_b, word in (([0, 130, 1], None, None, "column 130 is a pad or retired column"), ([0, 1], b, [2, 33], "column 33 is a pad or retired column"),
                                      ([0, 78], a, None, "column 78 is a pad or retired column")):
        with pytest.raises(ka.KwageError) as e:
            a.g.column_neighbors(3, cols, other.g if other else None, cols_b)
        assert e.value.code == ERR_ARG and word in e.value.message and "kwage_group_column_neighbors_device" in e.value.message
        with pytest.raises(ka.KwageError) as e:
            a.g.column_neighbors_host(3, cols, other.g if other else None, cols_b)
        assert word in e.value.message


def test_min_shared(ka, world):
    a, b, rng = world
    cells = om.of_models(a.m, None, b.m, None).astype(np.int64)
    live = cells[np.flatnonzero(a.m.real)][:, np.flatnonzero(b.m.real)]
    cut = int(np.sort(live.max(axis=1))[len(live) // 3])         # a third of the rows have no cell that large
    for metric in METRICS:
        rec, cnt, _ = check(a, None, b, None, k=4, metric=metric, min_shared=cut)
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < 4)).any() and (rec[:, :, 1][rec[:, :, 0] != 0xFFFFFFFF] >= cut).all()


# ------------------------------------------------------------------------------------------------------------------
# strips and parts: the same arrays however the work is cut
# ------------------------------------------------------------------------------------------------------------------

def test_strips_and_parts_give_the_same_lists(ka, ctx, world):
    a, b, rng = world
    la = om.list_of(rng, "shuffle", a.m.real, 300)
    lb = om.list_of(rng, "mixed", b.m.real)
    seen = []
    for metric in METRICS:
        want = nm.of_models(a.m, la, None, None, 9, metric, 0, True)
        want_b = nm.of_models(a.m, la, b.m, lb, 9, metric)
        want_null = nm.of_models(a.m, None, b.m, lb, 9, metric)
        for strip_bytes, entries, strips in ((128 * 300 * 4, 128, 3), (256 * 300 * 4 + 1000, 256, 2), (STRIP_BYTES, 300, 1)):
            for splits in (1, 2, 8):
                with ctx.tuning(neighbors_strip_bytes=strip_bytes, overlap_splits=splits):
                    rec, cnt, st = check(a, la, k=9, metric=metric, skip_self=True, strip_bytes=strip_bytes, want=want)
                    assert (st["strips"], st["strip_entries"], st["tiles"]) == (strips, entries, 9)
                    assert st["kernel"] == ("overlap_mfma_kernel+neighbors_select_kernel" if splits == 1 else "overlap_mfma_kernel+overlap_combine_kernel+neighbors_select_kernel")
        # against another group, and a NULL list of a (straight blocks with dead columns inside the strips)
        for strip_bytes in (128 * 100 * 4, 256 * 100 * 4, STRIP_BYTES):
            with ctx.tuning(neighbors_strip_bytes=strip_bytes):
                _, _, st = check(a, la, b, lb, k=9, metric=metric, strip_bytes=strip_bytes, want=want_b)
                _, _, st2 = check(a, None, b, lb, k=9, metric=metric, strip_bytes=strip_bytes, want=want_null)
                assert st2["strips"] == (a.m.span + st2["strip_entries"] - 1) // st2["strip_entries"] and (st["strips"] > 1) == (strip_bytes != STRIP_BYTES)
        seen.append(want)
    assert not np.array_equal(seen[0][0], seen[1][0])


# ------------------------------------------------------------------------------------------------------------------
# state: an open tail, after finalize, a fold, a group emptied by compaction
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 33, 129])
def test_an_open_tail_and_finalize(ka, ctx, n):
    rng = np.random.default_rng(n)
    L = 6
    a = Pair(ka, ctx, L, 600)
    try:
        a.insert(gm.random_filters(rng, L, n))
        assert a.m.span == (n + 7) // 8 * 8
        for metric in METRICS:
            check(a, None, k=3, metric=metric, skip_self=True)
            check(a, [n - 1], same_as_a=True, cols_b=None, k=3, metric=metric)
        a.finalize()
        for metric in METRICS:
            rec, cnt, _ = check(a, None, k=3, metric=metric)
            bits = a.g.column_bits()
            live = np.flatnonzero(a.m.real)
            assert np.array_equal(rec[live, 0, 2], bits[live])
    finally:
        a.close()


def test_a_fold(ka, world):
    a, b, rng = world
    fa, _ = a.g.fold(7)
    fb, _ = b.g.fold(7)
    try:
        pa, pb = Pair.__new__(Pair), Pair.__new__(Pair)
        pa.g, pa.m = fa, a.m.fold(7)[0]
        pb.g, pb.m = fb, b.m.fold(7)[0]
        check(pa, om.list_of(rng, "mixed", a.m.real), pb, None, k=6)
        check(pa, None, k=6, metric=nm.SHARED, skip_self=True)
    finally:
        fa.close()
        fb.close()


def test_a_group_emptied_by_a_compaction(ka, ctx):
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
        for other in (None, a, b):
            rec, cnt, st = check(a, None, other, None, k=3)
            assert rec.shape == (0, 3, 4) and (st["n_a"], st["strips"], st["kernel"]) == (0, 0, "")
        rec, cnt, st = check(b, None, a, None, k=3)             # no candidate: counts of 0, filler records
        assert rec.shape == (8, 3, 4) and not cnt.any() and (rec == nm.FILLER).all() and st["kernel"] == "neighbors_select_kernel"
        a.insert(gm.random_filters(rng, L, 3))                  # and it lives on
        check(a, None, b, None, k=3)
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
        out = torch.full((3, 2, 4), om.SENTINEL, dtype=torch.int32, device="cuda")
        counts = torch.full((3,), om.SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        free = ctx.mem_info()[0]
        good = (C.c_uint64 * 3)(0, 1, 2)
        beyond = (C.c_uint64 * 3)(0, 100000, 130)               # (the later faults every earlier refusal carries)

        def call(ga, ca, na, gb, cb, nb, k=0, metric=9, o=True, c=True):
            st = native.NeighborsStats(n_a=77, tiles=77, kernel_ms=-1.0)
            rc = lib.kwage_group_column_neighbors_device(ga, ca, na, gb, cb, nb, k, metric, 0, out.data_ptr() if o else None, counts.data_ptr() if c else None,
                                                         2 | 0x100, C.byref(st))
            assert (st.n_a, st.tiles, st.kernel_ms) == (77, 77, -1.0)
            return rc, lib.kwage_last_error()

        def refused(got, status, word):
            assert got[0] == status and word in got[1] and b"kwage_group_column_neighbors_device" in got[1], (got, word)

        A, B = a.g._h, b.g._h
        refused(call(None, None, 3, foreign._h, beyond, 0, o=False, c=False), ERR_ARG, b"NULL a")
        refused(call(A, None, 3, foreign._h, beyond, 0, o=False, c=False), ERR_ARG, b"NULL out")
        refused(call(A, None, 3, foreign._h, beyond, 0, c=False), ERR_ARG, b"NULL counts")
        refused(call(A, None, 3, foreign._h, beyond, 0), ERR_ARG, b"k = 0")
        refused(call(A, None, 3, foreign._h, beyond, 0, k=1025), ERR_ARG, b"k = 1025")
        refused(call(A, None, 3, foreign._h, beyond, 0, k=2), ERR_ARG, b"unknown metric 9")
        ok = dict(k=2, metric=1)
        refused(call(A, None, 3, foreign._h, beyond, 0, **ok), ERR_ARG, b"NULL cols_a with n_a = 3")
        refused(call(A, beyond, 0, foreign._h, beyond, 0, **ok), ERR_ARG, b"n_a is 0")
        refused(call(A, beyond, 3, foreign._h, None, 3, **ok), ERR_ARG, b"NULL cols_b with n_b = 3")
        refused(call(A, beyond, 3, foreign._h, beyond, 0, **ok), ERR_ARG, b"n_b is 0")
        refused(call(A, beyond, 3, None, beyond, 3, **ok), ERR_ARG, b"cols_b without b")
        refused(call(A, beyond, 3, foreign._h, beyond, 3, **ok), ERR_ARG, b"different contexts")
        refused(call(A, beyond, 3, sparse._h, beyond, 3, **ok), ERR_ARG, b"sparse")
        refused(call(sparse._h, beyond, 3, A, beyond, 3, **ok), ERR_ARG, b"sparse")
        refused(call(sparse._h, beyond, 3, None, None, 0, **ok), ERR_ARG, b"sparse")
        for g, word in zip(differing, (b"kmer_len", b"num_hash", b"log_2_filter_len")):
            refused(call(A, beyond, 3, g._h, beyond, 3, **ok), ERR_ARG, word)
            refused(call(g._h, beyond, 3, A, beyond, 3, **ok), ERR_ARG, word)
        pending = searched.submit(batch, 1.0)
        got = [call(A, beyond, 3, B, beyond, 3, **ok), call(A, beyond, 3, None, None, 0, **ok)]
        pending.collect()
        ctx.sync()
        refused(got[0], ERR_STATE, b"pending")
        refused(got[1], ERR_STATE, b"pending")
        refused(call(A, beyond, 3, B, beyond, 3, **ok), ERR_ARG, b"column 100000 is at or beyond the span %d" % a.g.column_span)
        refused(call(A, (C.c_uint64 * 3)(0, 130, 100000), 3, B, beyond, 3, **ok), ERR_ARG, b"column 130 is a pad or retired column")
        refused(call(A, good, 3, B, beyond, 3, **ok), ERR_ARG, b"column 100000 is at or beyond the span %d" % b.g.column_span)
        refused(call(A, good, 3, B, (C.c_uint64 * 3)(0, 33, 100000), 3, **ok), ERR_ARG, b"column 33 is a pad or retired column")
        refused(call(A, beyond, 3, None, None, 0, **ok), ERR_ARG, b"column 100000")
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == om.SENTINEL).all() and (counts.cpu().numpy() == om.SENTINEL).all() and ctx.mem_info()[0] == free
        # and the same call succeeds afterwards, a column listed twice, without stats too
        assert lib.kwage_group_column_neighbors_device(A, (C.c_uint64 * 3)(0, 1, 0), 3, B, good, 3, 2, 1, 0, out.data_ptr(), counts.data_ptr(), 0, None) == 0
        want = nm.of_models(a.m, [0, 1, 0], b.m, [0, 1, 2], 2, nm.JACCARD)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(counts.cpu().numpy().view(np.uint32), want[1])
        with pytest.raises(ValueError):
            a.g.column_neighbors(2, [0], None, [1])
        with pytest.raises(ValueError):
            a.g.column_neighbors(2, [0], metric="cosine")
    finally:
        batch.close()
        for g in [sparse, searched, foreign] + differing:
            g.close()
        other_ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# FileDatabase.sample_neighbors and kwage_neighbors, on the golden `.db` files
# ------------------------------------------------------------------------------------------------------------------

def db_samples(oracle, files):
    """[(accession, path, column in the file, parameters, bool column)] of `.db` files in the order given, read with the
    oracle's reader."""
    out = []
    for path in files:
        f = oracle.read_db(path)
        bits = np.unpackbits(np.asarray(f.rows), axis=1, bitorder="little")[:, :f.header.num_filter].astype(bool)
        key = (f.header.kmer_len, f.header.num_hash, f.header.log_2_filter_len, f.header.hash_func)
        out.extend((oracle.accession_to_str(f.info(j).run_accession), path, j, key, bits[:, j]) for j in range(f.header.num_filter))
    return out


def in_database_order(db, samples):
    """The samples in the database's order (group, then column), each with the accession the database reports."""
    at = {(s[1], s[2]): s for s in samples}
    out = [at[(path, c)] for _, _, path, c in db._samples()]
    assert len(out) == len(samples) and [s[0] for s in out] == [db._accession(path, c) for _, _, path, c in db._samples()]
    return out


def expected_lists(samples, k, accessions=None, metric=nm.JACCARD, min_shared=0):
    """([(accession, [(neighbour accession, path, column, shared, bits_query, bits_neighbour, jaccard)])], left-out
    accessions, whether distinct fractions met as equal doubles): the candidates are the samples with the first query's
    parameters, in the order given; a sample is never its own neighbour."""
    first = {}
    for place, s in enumerate(samples):
        first.setdefault(s[0], place)
    queries = list(range(len(samples))) if accessions is None else [first[a] for a in accessions]
    want = samples[queries[0]][3]
    left_out = [s[0] for s in samples if s[3] != want]
    cands = [p for p, s in enumerate(samples) if s[3] == want]
    m = np.stack([samples[p][4] for p in cands], axis=1).astype(np.int64)
    shared = m.T @ m
    bits = np.diag(shared)
    at = {p: i for i, p in enumerate(cands)}
    out, doubles_tie = [], False
    for q in queries:
        if samples[q][3] != want:
            continue
        i = at[q]
        found = []
        for j, p in enumerate(cands):
            s, union = int(shared[i, j]), int(bits[i] + bits[j] - shared[i, j])
            if p != q and s >= min_shared:
                key = s if metric == nm.SHARED else (Fraction(s, union) if union else Fraction(0))
                found.append((-key, p, (samples[p][0], samples[p][1], samples[p][2], s, int(bits[i]), int(bits[j]), s / union if union else 0.0)))
        found.sort(key=lambda t: t[:2])
        fracs = {}
        for key, _, rec in found:
            fracs.setdefault(rec[6], set()).add(key)
        doubles_tie = doubles_tie or (metric == nm.JACCARD and any(len(v) > 1 for v in fracs.values()))
        out.append((samples[q][0], [t[2] for t in found[:k]]))
    return out, left_out, doubles_tie


@pytest.mark.parametrize("metric", METRICS)
def test_sample_neighbors_on_the_golden_files(ka, ctx, oracle, golden_dir, metric):
    db = ka.FileDatabase(ctx, [os.path.join(golden_dir, "basic", "db")])
    try:
        samples = in_database_order(db, db_samples(oracle, db.files))
        order = [s[0] for s in samples]
        want, left_out, doubles_tie = expected_lists(samples, 5, metric=metric)
        assert not left_out and db.sample_neighbors(5, metric=metric) == want
        pick = [order[5], order[0], order[17], order[5]]
        want, _, _ = expected_lists(samples, 3, pick, metric=metric, min_shared=1)
        got = db.sample_neighbors(3, pick, metric=metric, min_shared=1)
        assert got == want and [a for a, _ in got] == pick
        if metric == nm.JACCARD:
            # the filter search's lists, the sample itself taken out: at these filter lengths distinct fractions are distinct doubles
            assert not doubles_tie
            want, _, doubles_tie = expected_lists(samples, 4, pick)
            assert not doubles_tie
            similar = db.similar_samples(pick, 5)
            me = {s[0]: (s[1], s[2]) for s in reversed(samples)}
            trimmed = [(a, [r for r in lst if (r[1], r[2]) != me[a]][:4]) for a, lst in similar]
            assert db.sample_neighbors(4, pick) == trimmed == want
        with pytest.raises(KeyError):
            db.sample_neighbors(3, ["SRR0000000"])
    finally:
        db.close()
    # several groups: the candidates are the groups of one parameter set, the others left out and named
    db = ka.FileDatabase(ctx, [os.path.join(golden_dir, "multi", "dbs")])
    try:
        assert len(db.groups) >= 2
        samples = in_database_order(db, db_samples(oracle, db.files))
        want, left_out, _ = expected_lists(samples, 6, metric=metric)
        assert left_out
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = db.sample_neighbors(6, metric=metric)
        assert got == want
        assert len(w) == 1 and all(a in str(w[0].message) for a in left_out)
    finally:
        db.close()


def golden_files(root):
    out = []
    for d, _, names in os.walk(root):
        out.extend(os.path.join(d, n) for n in names if n.endswith(".db"))
    return sorted(out)


@pytest.mark.parametrize("metric", METRICS)
def test_kwage_neighbors(ka, oracle, golden_dir, tmp_path, metric):
    from kwage_amd import native
    tool = os.path.join(os.path.dirname(native.KWAGE_DBTOOL_BIN), "kwage_neighbors")
    root = os.path.join(golden_dir, "multi", "dbs")
    flags = ["--shared"] if metric == nm.SHARED else []
    HEAD = ["sample", "neighbour", "rank", "shared", "bits_sample", "bits_neighbour", "jaccard"]

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    def lines_of(want):
        return [[a, r[0], str(rank + 1), str(r[3]), str(r[4]), str(r[5]), "%.6f" % r[6]] for a, lst in want for rank, r in enumerate(lst)]

    # argument errors end the program before a device is opened
    r = run()
    assert r.returncode == 1 and "Usage for kwage_neighbors" in r.stderr
    r = run("-d", root)
    assert r.returncode == 1 and not r.stdout and r.stderr
    r = run("-d", root, "-k", "0")
    assert r.returncode == 1 and not r.stdout
    r = run("-d", root, "-k", "3", "--min-shared", "x")
    assert r.returncode == 1 and "--min-shared" in r.stderr
    r = run("-d", root, "-k", "3", "-s", "SRR0000000")
    assert r.returncode == 1 and "SRR0000000" in r.stderr and not r.stdout
    r = run("-d", str(tmp_path), "-k", "3")
    assert r.returncode == 1 and "Please provide at least one database file" in r.stderr
    # every sample: the program's file order is the directory walk's -- the order of the querying samples in its output
    out = str(tmp_path / "neighbors.tsv")
    r = run("-d", root, "-k", "4", "-o", out, *flags)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("Skipping ") >= 1
    rows = [x.split("\t") for x in open(out).read().splitlines()]
    assert rows[0] == HEAD
    by_file = {}
    for s in db_samples(oracle, golden_files(root)):
        by_file.setdefault(s[1], []).append(s)
    acc_file = {s[0]: p for p, ss in by_file.items() for s in reversed(ss)}
    file_order = []
    for x in rows[1:]:
        if acc_file[x[0]] not in file_order:
            file_order.append(acc_file[x[0]])
    kept = [s for p in file_order for s in by_file[p]]
    want, left_out, _ = expected_lists(kept, 4, metric=metric)
    assert not left_out and rows[1:] == lines_of(want)
    # listed samples, positional and with -s, a repeat among them; --min-shared
    names = [s[0] for s in kept]
    pick = [names[3], names[1], names[3]]
    cut = int(want[3][1][1][3])                                 # the shared bits of the second neighbour of names[3]
    r = run("-d", root, "-k", "2", "--min-shared", str(cut), "-s", pick[0], pick[1], pick[2], *flags)
    assert r.returncode == 0, r.stderr
    rows = [x.split("\t") for x in r.stdout.splitlines()]
    want, _, _ = expected_lists(kept, 2, pick, metric=metric, min_shared=cut)
    assert rows[0] == HEAD and rows[1:] == lines_of(want) and [a for a, _ in want] == pick
