"""Compaction (include/kwage_amd.h: kwage_group_compact; Group.compact, FileDatabase.compact): the gaps that retired
columns and alignment pads leave in a RESIDENT group closed in place.

The expected matrix is numpy's, never the code under test: np.packbits(image[:, valid], axis=1, bitorder="little"), the
expected map the rank among the valid columns, the expected stats the plan restated in tests/compact_cases.py; the
expected search results are the oracle's on the survivors' image (test_gpu_live_insert.py's check_all_forms).  Every
comparison is exact equality.  The cases are data: tests/compact_cases.py."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN

import compact_cases as cc
import test_gpu_live_insert as li

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
K, NH = 21, 2
GUARD = 0x5A5A5A5A5A5A5A5A


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


def compact_abi(g, capacity=None, timing=True, want_map=True):
    """kwage_group_compact through ctypes -> (status, int64 map of `capacity` entries + 2 guard entries, stats)"""
    from kwage_amd import native
    span = g.column_span
    capacity = span if capacity is None else capacity
    new = np.full(max(span, capacity) + 2, GUARD, dtype=np.uint64)
    st = native.CompactStats(span_before=GUARD, kernel_ms=-1.0)
    rc = native.lib().kwage_group_compact(g._h, 2 if timing else 0, new.ctypes.data_as(C.POINTER(C.c_uint64)) if want_map else None,
                                          capacity, C.byref(st))
    return rc, new.view(np.int64), st


def filters_of(img, columns):
    """uint8 [n, max(1, nrows / 8)]: the listed columns of the image as Bloom filters (filter-major, LSB first)."""
    return np.ascontiguousarray(np.packbits(img[:, columns].T, axis=1, bitorder="little"))


def build(ka, ctx, case, L, finalized):
    """The case's group before the compaction, its image with the retired columns cleared, and its layout."""
    lay = cc.layout(case)
    nrows = 1 << L
    img = cc.image(case, nrows, seed=L)
    g = ka.Group(ctx, K, NH, L, lay.capacity)
    at = 0
    for n in case.blocks:
        first = lay.columns[at]
        block = np.ascontiguousarray(np.packbits(img[:, first:first + n], axis=1, bitorder="little"))
        assert g.add_columns(block, n) == first
        at += n
    if finalized and not case.inserts:
        g.finalize()
    for n in case.inserts:
        assert g.insert_filters(filters_of(img, lay.columns[at:at + n])) == lay.columns[at]
        at += n
    if finalized and case.inserts:
        g.finalize()
    assert g.column_span == lay.span and at == len(lay.columns)
    if lay.retired:
        g.retire_columns(lay.retired)
        img[:, lay.retired] = False
    assert np.array_equal(g.read_rows(np.arange(nrows)), np.packbits(img, axis=1, bitorder="little"))
    return g, img, lay


SIZED = [cc.sized(c, r) for c in cc.CASES for r in (cc.RESIDUES if c.grow is not None else cc.RESIDUES[:1])]


@pytest.mark.parametrize("finalized", [False, True], ids=["open", "finalized"])
@pytest.mark.parametrize("L", [0, 8])
@pytest.mark.parametrize("case", SIZED, ids=lambda c: "%s-%d" % (c.name, sum(c.blocks)))
def test_case(ka, ctx, case, L, finalized):
    g, img, lay = build(ka, ctx, case, L, finalized)
    nrows = 1 << L
    rng = np.random.default_rng(len(lay.columns) + L)
    try:
        want = cc.reference(img, lay.valid)
        plan = cc.plan(lay)
        rc, new, st = compact_abi(g)
        assert rc == 0, rc
        assert np.array_equal(new[:lay.span], lay.new_column) and np.all(new[lay.span:].view(np.uint64) == GUARD)
        got_stats = {f: getattr(st, f) for f in plan}
        assert got_stats == plan, (got_stats, plan)
        assert (st.kernel_ms > 0) == (plan["units"] > 0), st.kernel_ms
        assert g.column_span == plan["span_after"] and g.row_bytes == (lay.m + 7) // 8 and g.num_columns == lay.m
        if lay.m:
            got = g.read_rows(np.arange(nrows))
            assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        # again, through the Python mirror: nothing is left to close -- the identity map, no kernel, the same matrix
        again, st2 = g.compact(timing=True)
        assert again.dtype == np.int64 and again.shape == (plan["span_after"],)
        assert np.array_equal(again[:lay.m], np.arange(lay.m)) and np.all(again[lay.m:] == -1)
        assert st2["units"] == 0 and st2["kernel_ms"] == 0 and st2["columns"] == lay.m and st2["span_after"] == st2["span_before"] == plan["span_after"]
        assert np.array_equal(g.real_columns(), np.arange(plan["span_after"]) < lay.m)
        if lay.m:
            assert np.array_equal(g.read_rows(np.arange(nrows)), want)
        if finalized and lay.m:
            assert np.array_equal(g.column_bits(), np.concatenate([img[:, lay.valid].sum(axis=0), np.zeros(plan["span_after"] - lay.m, dtype=np.int64)]).astype(np.uint32))
        # the tail is open at m: the next insert continues at bit granularity
        more = max(case.after, 1)
        fresh = rng.random((nrows, more)) < 0.5
        assert g.insert_filters(filters_of(fresh, list(range(more)))) == lay.m
        image = li.Image(L)
        image.put(0, np.concatenate([img[:, lay.valid], fresh], axis=1))
        li.check_rows(g, image)
        if not finalized:                           # and everything from there to the stride is zero
            li.check_zero_to_the_stride(ka, g, image)
    finally:
        g.close()


def test_searches_before_and_after(ka, ctx, oracle):
    k, nh, L = 15, 2, 8
    rng = np.random.default_rng(17)
    queries = [li.random_dna(rng, 16) for _ in range(14)] + [li.random_dna(rng, 40), li.random_dna(rng, 90)]
    a, b = rng.random((1 << L, 150)) < 0.6, rng.random((1 << L, 77)) < 0.5
    filters = li.random_filters(rng, L, 30)
    image = li.Image(L)
    g = ka.Group(ctx, k, nh, L, 2000)
    try:
        image.put(g.add_columns(np.packbits(a, axis=1, bitorder="little"), 150), a)
        image.put(g.add_columns(np.packbits(b, axis=1, bitorder="little"), 77), b)
        g.finalize()
        first = g.insert_filters(filters)
        image.put(first, li.columns_of(filters, L))
        gone = [0, 31, 32, 149, 256 + 5, 256 + 76, first + 2, first + 29]
        g.retire_columns(gone)
        for c in gone:
            image.retire(c)
        before = li.check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, [8, 256, first + 3])
        new, st = g.compact()
        m = int(image.real.sum())
        assert st["columns"] == m == 150 + 77 + 30 - 8 and st["span_before"] == image.span and st["runs"] == 6
        assert np.array_equal(new, np.where(image.real, np.cumsum(image.real) - 1, -1))
        after_image = li.Image(L)
        after_image.put(0, image.bits[:, image.real])
        li.check_rows(g, after_image)
        after = li.check_all_forms(ka, oracle, g, after_image, ctx, k, nh, L, queries, [int(new[c]) for c in (8, 256, first + 3)])
        for t in (1.0, 0.8):                        # identical after mapping columns through new_column
            assert before[t] and [(q, int(new[c]), n) for q, c, n in before[t]] == after[t]
        assert not any(ctx.scratch_nonzero().values())
    finally:
        g.close()


def test_capacity_comes_back(ka, ctx):
    from kwage_amd.native import lib
    L, k5 = 6, 5
    rng = np.random.default_rng(18)
    g = ka.Group(ctx, K, NH, L, 1000)
    try:
        cap = 8 * g.row_stride
        cols = rng.random((1 << L, cap)) < 0.5
        assert g.insert_filters(filters_of(cols, list(range(cap)))) == 0
        g.finalize()
        fresh = rng.random((1 << L, k5)) < 0.5
        extra = filters_of(fresh, list(range(k5)))
        first = C.c_uint64(77)
        before = li.state_of(g, 1 << L)
        rc = lib().kwage_group_insert_filters(g._h, extra.ctypes.data, extra.strides[0], k5, 0, C.byref(first), None)
        assert rc == ERR_ARG and b"capacity" in lib().kwage_last_error() and first.value == 77
        assert li.same_state(li.state_of(g, 1 << L), before)
        gone = [0, 127, 128, 500, cap - 1]
        g.retire_columns(gone)
        rc = lib().kwage_group_insert_filters(g._h, extra.ctypes.data, extra.strides[0], k5, 0, C.byref(first), None)
        assert rc == ERR_ARG and b"capacity" in lib().kwage_last_error()          # retire alone gives nothing back
        new, st = g.compact()
        assert st["columns"] == cap - k5 and st["span_after"] == (cap - k5 + 7) // 8 * 8
        assert g.insert_filters(extra) == cap - k5 and g.column_span == cap and g.num_columns == cap
        keep = np.ones(cap, dtype=bool)
        keep[gone] = False
        want = np.packbits(np.concatenate([cols[:, keep], fresh], axis=1), axis=1, bitorder="little")
        assert np.array_equal(g.read_rows(np.arange(1 << L)), want)
    finally:
        g.close()


def test_save_before_equals_save_after(ka, ctx, tmp_path):
    case = cc.sized(cc.CASES[5], 1)                 # holes across 32-bit and 128-bit boundaries
    g, img, lay = build(ka, ctx, case, 8, True)
    try:
        survivors = np.flatnonzero(lay.valid).tolist()
        sources = [{"run_accession": "SRR%d" % (j + 1)} for j in range(lay.m)]
        a, b = str(tmp_path / "before.db"), str(tmp_path / "after.db")
        g.save_db(a, survivors, sources)
        g.compact()
        g.save_db(b, list(range(lay.m)), sources)
        assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > (1 << 8) * ((lay.m + 7) // 8)
    finally:
        g.close()


def test_refusals_leave_everything_as_it_was(ka, ctx):
    from kwage_amd.native import lib
    case = cc.CASES[5]
    L = 8
    g, img, lay = build(ka, ctx, case, L, True)
    rng = np.random.default_rng(19)
    sparse = ka.Group.sparse(ctx, K, NH, L, 300, np.arange(0, 1 << L, 2))
    try:
        before = li.state_of(g, 1 << L)
        bits = g.column_bits().copy()

        def untouched():
            g._column_bits = None
            return li.same_state(li.state_of(g, 1 << L), before) and np.array_equal(g.column_bits(), bits)

        for capacity in (0, 1, lay.span - 1):       # a short map
            rc, new, st = compact_abi(g, capacity=capacity)
            assert rc == ERR_ARG and b"new_column" in lib().kwage_last_error()
            assert np.all(new.view(np.uint64) == GUARD) and st.span_before == GUARD and untouched()
        block = np.ascontiguousarray(rng.integers(0, 256, size=(1 << (L - 1), 3), dtype=np.uint8))
        assert sparse.add_columns(block, 20) == 0
        sparse_before = sparse.read_rows(np.arange(1 << (L - 1)))
        rc, new, st = compact_abi(sparse)
        assert rc == ERR_ARG and b"sparse" in lib().kwage_last_error() and np.all(new.view(np.uint64) == GUARD)
        assert sparse.column_span == 24 and sparse.num_columns == 20 and np.array_equal(sparse.read_rows(np.arange(1 << (L - 1))), sparse_before)
        b = ka.Batch(ctx, [li.random_dna(rng, 30) for _ in range(8)])
        try:
            pending = g.submit(b, 1.0)
            rc, new, st = compact_abi(g)
            pending.collect()
            assert rc == ERR_STATE and b"pending" in lib().kwage_last_error() and np.all(new.view(np.uint64) == GUARD)
            assert untouched()
        finally:
            b.close()
        # and the group still compacts; without a map and without stats too
        assert lib().kwage_group_compact(g._h, 0, None, 0, None) == 0
        assert g.column_span == (lay.m + 7) // 8 * 8 and np.array_equal(g.read_rows(np.arange(1 << L)), cc.reference(img, lay.valid))
    finally:
        g.close()
        sparse.close()


def test_file_database(ka, ctx, oracle, tmp_path):
    # (score_matrix imports torch: where this is the process's first use of it, its start-up of ~10 s is counted here;
    # the test's own work takes a fraction of a second)
    dbs = os.path.join(GOLDEN, "multi", "dbs")
    rng = np.random.default_rng(20)
    fresh = [li.random_dna(rng, 400) for _ in range(3)]
    reads = [s for _, s in oracle.read_sequences(os.path.join(GOLDEN, "multi", "reads.fastq"))][:4]
    queries = reads + [fresh[0][30:200], fresh[1][100:300], fresh[0][:60] + fresh[1][:60], fresh[2][5:150]]

    def answers(db, all_forms=True):
        out = {}
        for t in (1.0, 0.8):
            out["hits", t] = [(h.query, h.path, h.column, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences(queries, t)]
        s, acc = db.score_matrix(queries)
        out["scores"] = (s.tolist(), acc)
        if not all_forms:
            return out
        p, acc = db.presence_matrix(queries, 0.8)
        out["presence"] = (p.tolist(), acc)
        out["top"] = [(h.query, h.path, h.column, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences_top(queries, 4)]
        out["near"] = db.similar_samples([acc[1], "SRR9999002"], 3)
        return out

    db = ka.FileDatabase(ctx, [dbs], headroom=64)
    try:
        base_acc = db.score_matrix(queries[:1])[1]
        assert db.add_sample("SRR9999001", [fresh[0]])[0] == 0
        assert db.add_sample("SRR9999002", [fresh[1]])[0] == 0
        # a file sample with neighbours on both sides: its file becomes two pieces of the layout
        wide = [oracle.read_db(f) for f in db.files if oracle.read_db(f).header.num_filter >= 3][0]
        victim = wide.info(1).csv_string()
        assert base_acc.count(victim) == 1
        gi, col = db.retire_sample(victim)
        db.retire_sample("SRR9999001")
        spans = [g.column_span for g in db.groups]
        counts = [g.num_columns for g in db.groups]
        want = answers(db)
        assert any(a == "SRR9999002" for _, _, _, a, _, _ in want["hits", 1.0]) and victim not in want["scores"][1]
        stats = db.compact()
        assert [s["columns"] for s in stats] == counts == [g.num_columns for g in db.groups]
        assert [g.column_span for g in db.groups] == [(n + 7) // 8 * 8 for n in counts] and sum(g.column_span for g in db.groups) < sum(spans)
        got = answers(db)
        assert got == want
        # retire and add go on as before: a further sample lands right behind group 0's survivors
        assert db.add_sample("SRR9999003", [fresh[2]]) == (0, counts[0])
        assert db.retire_sample("SRR9999002")[0] == 0
        db.add_sample("SRR9999002", [fresh[1]])     # (back in, behind SRR9999003)
        with pytest.raises(KeyError):
            db.retire_sample(victim)
        final = answers(db, all_forms=False)
        assert any(a == "SRR9999003" for _, _, _, a, _, _ in final["hits", 1.0])
        written = db.save(str(tmp_path / "saved"))
    finally:
        db.close()
    again = ka.FileDatabase(ctx, [str(tmp_path / "saved")])
    try:
        assert written and sum(g.num_columns for g in again.groups) == sum(counts) + 1
        for t in (1.0, 0.8):
            got = Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in again.search_sequences(queries, t))
            assert got == Counter((q, a, f, n) for q, _, _, a, f, n in final["hits", t]), t
        s, acc = again.score_matrix(queries)
        assert Counter(zip(acc, map(tuple, s.T.tolist()))) == Counter(zip(final["scores"][1], map(tuple, np.array(final["scores"][0]).T.tolist())))
    finally:
        again.close()
