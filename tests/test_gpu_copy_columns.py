"""The copy between groups (include/kwage_amd.h: kwage_group_copy_columns; Group.copy_columns_from, FileDatabase.reserve,
FileDatabase.merge_groups): listed columns of one RESIDENT group packed into another one's rows on the device.

The expected matrix is numpy's, never the code under test: the destination's image with the source image's listed columns
put at the insert's place; the expected state is that of a TWIN of the destination that received
insert_filters(src.export_filters(cols)); the expected search results are the oracle's on the image.  Every comparison is
exact equality.  The sources are the compaction's cases (tests/compact_cases.py through test_gpu_compact.build): file
blocks, inserts at bit offsets, retired columns, and bits planted in dead columns."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import compact_cases as cc
import test_gpu_compact as tc
import test_gpu_live_insert as li

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
K, NH, L = tc.K, tc.NH, 8
NROWS = 1 << L
GUARD = 0x5A5A5A5A5A5A5A5A
STAT_FIELDS = ("first_column", "columns", "runs", "first_unit", "units", "bytes_written")


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
# sources, lists, destinations
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sources(ka, ctx):
    """case name -> (group, image with bits planted in dead columns ignored, layout, state): built once, never changed --
    every test that reads one checks at its end that the state is still this one."""
    made = {}

    def get(case):
        if case.name not in made:
            g, img, lay = tc.build(ka, ctx, case, L, finalized=case.name in "bdfj")
            dead = np.flatnonzero(~lay.valid)
            if dead.size:                           # bits planted in pad and retired columns: they must not travel
                rng = np.random.default_rng(lay.span)
                rows = rng.integers(0, NROWS, size=4 * dead.size)
                g.set_bits(rows, np.tile(dead, 4))
            made[case.name] = (g, img, lay, li.state_of(g, NROWS))
        return made[case.name]
    yield get
    for g, _, _, _ in made.values():
        g.close()


def lists_of(case, lay):
    """name -> the column list (None: the all-columns form) for a source whose valid columns are lay.valid."""
    v = np.flatnonzero(lay.valid)
    rng = np.random.default_rng(7 + lay.m)
    out = {"all": None, "reversed": v[::-1], "every-other": v[::2], "shuffled": rng.permutation(v), "one": v[lay.m // 2:lay.m // 2 + 1]}
    if lay.m > 129:
        out["boundaries"] = v[[31, 32, 127, 128, 129]]
    if case.name == "a":
        out["ascending"] = v                        # all of a 70 000-column block but one: more than 256 units per row
    return out


TAILS = (1, 31, 32, 33, 127, 0)
DESTS = ["fresh", "block70"] + ["%s-%d" % (kind, r) for r in TAILS for kind in ("open", "planted", "final") if kind != "planted" or r % 8]


def make_dest(ka, ctx, dest, capacity):
    """The destination (or its twin: the same calls, the same seed) -> (group, image, where the next insert lands)."""
    rng = np.random.default_rng(len(dest) + 100 * sum(map(ord, dest)))
    g = ka.Group(ctx, K, NH, L, capacity)
    image = li.Image(L)
    if dest == "fresh":
        return g, image, 0
    if dest == "block70":
        cols = rng.random((NROWS, 70)) < 0.5
        assert g.add_columns(np.ascontiguousarray(np.packbits(cols, axis=1, bitorder="little")), 70) == 0
        image.put(0, cols)
        return g, image, 128                        # a block closes the tail: the next 16-byte boundary
    kind, r = dest.split("-")
    tail = int(r) or 128
    cols = rng.random((NROWS, tail)) < 0.5
    assert g.insert_filters(tc.filters_of(cols, list(range(tail)))) == 0
    image.put(0, cols)
    if kind == "planted":                           # bits in the pad columns between the open tail and the span
        pads = np.arange(tail, image.span)
        assert pads.size
        rows = rng.integers(0, NROWS, size=8 * pads.size)
        g.set_bits(rows, np.tile(pads, 8))
        image.bits[rows, np.tile(pads, 8)] = True
    if kind == "final":
        g.finalize()
    return g, image, tail


def copy_abi(dst, src, cols, timing):
    """kwage_group_copy_columns through ctypes -> (status, first_column, stats)"""
    from kwage_amd import native
    first = C.c_uint64(GUARD)
    st = native.CopyStats(first_column=GUARD, units=GUARD, kernel_ms=-1.0)
    if cols is None:
        ptr, n = None, 0
    else:
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        ptr, n = cols.ctypes.data_as(C.c_void_p), cols.size
    rc = native.lib().kwage_group_copy_columns(dst._h, src._h, ptr, n, 2 if timing else 0, C.byref(first), C.byref(st))
    return rc, first.value, st


CASES = [c for c in cc.CASES if cc.layout(c).m]


@pytest.mark.parametrize("dest", DESTS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_copy(ka, ctx, sources, case, dest):
    src, img, lay, src_state = sources(case)
    valid = np.flatnonzero(lay.valid)
    for i, (name, cols) in enumerate(lists_of(case, lay).items()):
        listed = valid if cols is None else np.asarray(cols)
        n = int(listed.size)
        capacity = 256 + n + 200
        dst, image, first = make_dest(ka, ctx, dest, capacity)
        twin, _, _ = make_dest(ka, ctx, dest, capacity)
        try:
            timing = i % 2 == 0
            rc, got_first, st = copy_abi(dst, src, cols, timing)
            assert rc == 0, (name, rc)
            # the stats are what the shapes imply
            units = (first + n + 127) // 128 - first // 128
            want = {"first_column": first, "columns": n, "runs": int(1 + np.count_nonzero(np.diff(listed.astype(np.int64)) != 1)),
                    "first_unit": first // 128, "units": units, "bytes_written": NROWS * units * 16}
            assert got_first == first and {f: getattr(st, f) for f in STAT_FIELDS} == want, (name, got_first, want)
            assert (st.kernel_ms > 0) if timing else (st.kernel_ms == 0), (name, st.kernel_ms)
            # the matrix is numpy's (whatever was planted behind an open tail is overwritten)
            image.bits[:, first:] = False
            image.put(first, img[:, listed])
            li.check_rows(dst, image)
            # the state is the twin's, which took the same columns as filters
            assert twin.insert_filters(src.export_filters(listed)) == first
            dst._inserted(first, n)                  # (the call went around the Python mirror)
            assert li.same_state(li.state_of(dst, NROWS), li.state_of(twin, NROWS)), name
            if dest.startswith("final"):
                assert np.array_equal(dst.column_bits(), twin.column_bits())
            # a following insert lands right behind the copy
            more = np.random.default_rng(n).random((NROWS, 3)) < 0.5
            assert dst.insert_filters(tc.filters_of(more, [0, 1, 2])) == first + n, name
            image.put(first + n, more)
            li.check_rows(dst, image)
            if not dest.startswith("final"):         # everything from there to the stride is zero
                li.check_zero_to_the_stride(ka, dst, image)
        finally:
            dst.close()
            twin.close()
    assert li.same_state(li.state_of(src, NROWS), src_state)


def test_the_python_mirror(ka, ctx, sources):
    src, img, lay, src_state = sources(cc.CASES[-1])
    valid = np.flatnonzero(lay.valid)
    dst = ka.Group(ctx, K, NH, L, 4096)
    try:
        first, st = dst.copy_columns_from(src, timing=True)
        assert first == 0 and st["columns"] == lay.m and st["kernel_ms"] > 0 and set(st) == set(STAT_FIELDS) | {"kernel_ms"}
        first, st = dst.copy_columns_from(src, valid[5:9][::-1])
        assert first == lay.m and st["runs"] == 4 and st["kernel_ms"] == 0
        image = li.Image(L)
        image.put(0, img[:, valid])
        image.put(lay.m, img[:, valid[5:9][::-1]])
        li.check_rows(dst, image)
        assert np.array_equal(dst.real_columns(), image.real) and dst.room == 8 * dst.row_stride - lay.m - 4
        with pytest.raises(Exception):
            dst.copy_columns_from(src, [])            # an empty list is no all-columns form
    finally:
        dst.close()
    assert li.same_state(li.state_of(src, NROWS), src_state)


# ------------------------------------------------------------------------------------------------------------------
# the meaning: the copied columns answer every search as the samples they were built from
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def samples():
    """50 sequences of 300 bases and queries drawn from them plus random ones (shared, never changed)."""
    rng = np.random.default_rng(53)
    seqs = [li.random_dna(rng, 300) for _ in range(50)]
    picked = [int(c) for c in rng.permutation(40)[:17]]
    queries = [seqs[picked[0]][:80], seqs[picked[5]][100:260], seqs[picked[16]], seqs[41][10:40] + seqs[picked[3]][10:40], seqs[45][5:90],
               li.random_dna(rng, 60), li.random_dna(rng, 25), li.random_dna(rng, 21), li.random_dna(rng, 12)]
    return seqs, picked, queries


@pytest.mark.parametrize("nh", [1, 3, 5])
def test_meaning_and_searches(ka, ctx, oracle, samples, nh):
    seqs, picked, queries = samples
    k, lg = 21, 10
    filters = np.stack([oracle.bloom_bits_from_sequences([s], k, nh, lg) for s in seqs])
    src, dst = ka.Group(ctx, k, nh, lg, 64), ka.Group(ctx, k, nh, lg, 64)
    try:
        assert src.insert_filters(filters[:40]) == 0 and dst.insert_filters(filters[40:]) == 0
        dst.finalize()
        first, st = dst.copy_columns_from(src, picked)
        assert first == 10 and st["columns"] == 17 and st["runs"] == int(1 + np.count_nonzero(np.diff(picked) != 1))
        assert np.array_equal(dst.export_filters(list(range(27))), np.concatenate([filters[40:], filters[picked]]))
        image = li.Image(lg)
        image.put(0, li.columns_of(filters[40:], lg))
        image.put(10, li.columns_of(filters[picked], lg))
        li.check_rows(dst, image)
        b = ka.Batch(ctx, queries)
        try:
            for t in (1.0, 0.6):
                exp = li.oracle_hits(oracle, image, k, nh, lg, queries, t)
                assert t < 1 or any(q == 2 and c == 10 + 16 for q, c, _ in exp)
                for flags in (0, ka.SEARCH_EARLY_EXIT):
                    assert [tuple(h) for h in dst.search(b, t, flags).hits.tolist()] == exp, (t, flags)
        finally:
            b.close()
        li.check_all_forms(ka, oracle, dst, image, ctx, k, nh, lg, queries, [0, 26])
    finally:
        src.close()
        dst.close()


# ------------------------------------------------------------------------------------------------------------------
# refusals: found before a byte is written or allocated
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_write_and_allocate_nothing(ka, ctx, sources):
    from kwage_amd import native
    lib = native.lib()
    src, img, lay, src_state = sources(cc.CASES[-1])      # "j": blocks, pads, inserts, a retired column
    empty, _, elay, empty_state = sources(next(c for c in cc.CASES if c.name == "h"))
    assert elay.m == 0
    valid = np.flatnonzero(lay.valid)
    dead = np.flatnonzero(~lay.valid)
    rng = np.random.default_rng(71)
    dst = ka.Group(ctx, K, NH, L, 1024)
    sparse = ka.Group.sparse(ctx, K, NH, L, 1024, np.arange(0, NROWS, 2))
    differing = [ka.Group(ctx, K + 2, NH, L, 256), ka.Group(ctx, K, NH + 1, L, 256), ka.Group(ctx, K, NH, L - 1, 256)]
    searched = ka.Group(ctx, K, NH, L, 256)
    other_ctx = ka.Context(0)
    foreign = ka.Group(other_ctx, K, NH, L, 256)
    b = ka.Batch(ctx, [li.random_dna(rng, 30) for _ in range(8)])
    try:
        some = rng.random((NROWS, 37)) < 0.5
        assert dst.insert_filters(tc.filters_of(some, list(range(37)))) == 0
        for g in differing + [searched, foreign]:
            g.insert_filters(li.random_filters(rng, int(g.params.log_2_filter_len), 5))
        searched.finalize()
        searched.submit(b, 1.0).collect()           # (the context's search scratch exists from here on)
        ctx.sync()
        state = li.state_of(dst, NROWS)
        free = ctx.mem_info()[0]

        def refused(rc_first_st, status, word):
            rc, first, st = rc_first_st
            assert rc == status and word in lib.kwage_last_error(), (rc, lib.kwage_last_error())
            assert first == GUARD and st.first_column == GUARD and st.units == GUARD and st.kernel_ms == -1.0
            assert li.same_state(li.state_of(dst, NROWS), state)

        first = C.c_uint64(GUARD)
        cols = np.ascontiguousarray(valid[:3], dtype=np.uint64)
        ptr = cols.ctypes.data_as(C.c_void_p)
        for d, s, f in ((None, src._h, C.byref(first)), (dst._h, None, C.byref(first)), (dst._h, src._h, None)):
            assert lib.kwage_group_copy_columns(d, s, ptr, 3, 0, f, None) == ERR_ARG and b"NULL" in lib.kwage_last_error()
        assert lib.kwage_group_copy_columns(dst._h, src._h, None, 3, 0, C.byref(first), None) == ERR_ARG and b"NULL columns" in lib.kwage_last_error()
        assert lib.kwage_group_copy_columns(dst._h, src._h, ptr, 0, 0, C.byref(first), None) == ERR_ARG and b"n is 0" in lib.kwage_last_error()
        assert lib.kwage_group_copy_columns(dst._h, src._h, ptr, 1 << 32, 0, C.byref(first), None) == ERR_ARG and b"do not fit" in lib.kwage_last_error()
        assert first.value == GUARD
        refused(copy_abi(dst, empty, None, True), ERR_ARG, b"no valid column")
        refused(copy_abi(dst, dst, valid[:3], True), ERR_ARG, b"same group")
        refused(copy_abi(dst, foreign, [0, 1], True), ERR_ARG, b"different contexts")
        refused(copy_abi(dst, sparse, [0], True), ERR_ARG, b"sparse")
        refused(copy_abi(sparse, src, valid[:3], True), ERR_ARG, b"sparse")
        for g, word in zip(differing, (b"kmer_len", b"num_hash", b"log_2_filter_len")):
            refused(copy_abi(dst, g, [0, 1], True), ERR_ARG, word)
            refused(copy_abi(g, dst, [0, 1], True), ERR_ARG, word)
        # (hash_func: kwage_group_create accepts one hash function only, so no two groups can differ in it -- the refusal is
        # tests/sanitize/copy_sanitize.cpp's)
        refused(copy_abi(dst, src, [lay.span], True), ERR_ARG, b"beyond the span")
        refused(copy_abi(dst, src, [int(valid[0]), lay.span + 1000], True), ERR_ARG, b"beyond the span")
        refused(copy_abi(dst, src, [int(valid[0]), int(dead[0])], True), ERR_ARG, b"pad or retired")
        refused(copy_abi(dst, src, [int(lay.retired[0])], True), ERR_ARG, b"pad or retired")
        refused(copy_abi(dst, src, [int(valid[3]), int(valid[4]), int(valid[3])], True), ERR_ARG, b"listed twice")
        room = 8 * dst.row_stride - 37
        assert room < lay.m
        refused(copy_abi(dst, src, None, True), ERR_ARG, b"capacity exceeded")
        refused(copy_abi(dst, src, valid[:room + 1], True), ERR_ARG, b"capacity exceeded")
        pending = searched.submit(b, 1.0)
        out = copy_abi(dst, src, valid[:3], True)
        pending.collect()
        refused(out, ERR_STATE, b"pending")
        ctx.sync()
        assert ctx.mem_info()[0] == free
        # and the same copies succeed afterwards: to the last column of the row, without stats too
        rc, got_first, st = copy_abi(dst, src, valid[:3], True)
        assert rc == 0 and got_first == 37 and st.columns == 3
        full = np.ascontiguousarray(valid[3:room], dtype=np.uint64)
        assert lib.kwage_group_copy_columns(dst._h, src._h, full.ctypes.data_as(C.c_void_p), full.size, 0, C.byref(first), None) == 0 and first.value == 40
        image = li.Image(L)
        image.put(0, some)
        image.put(37, img[:, valid[:room]])
        assert image.span == 8 * dst.row_stride
        dst._inserted(37, room)
        li.check_rows(dst, image)
        assert li.same_state(li.state_of(src, NROWS), src_state) and li.same_state(li.state_of(empty, NROWS), empty_state)
    finally:
        b.close()
        for g in [dst, sparse, searched, foreign] + differing:
            g.close()
        other_ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# FileDatabase.reserve and FileDatabase.merge_groups
# ------------------------------------------------------------------------------------------------------------------

def build_dbs(ka, ctx, oracle, tmp_path, seqs, accs, files):
    """`.db` files under tmp_path/src from oracle-built `.bloom` files: files = [(name, log_2_filter_len, members)]."""
    from kwage_amd.native import lib, check, Params
    k, nh = 21, 2
    src = tmp_path / "src"
    src.mkdir()
    for name, lg, members in files:
        paths = []
        for i in members:
            p = str(tmp_path / ("%s_L%d.bloom" % (accs[i], lg)))
            oracle.write_bloom(p, k, lg, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession(accs[i])), oracle.bloom_bits_from_sequences([seqs[i]], k, nh, lg))
            paths.append(p)
        prm = Params(k, nh, lg, 0)
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        check(lib().kwage_build_db(ctx._h, str(src / name).encode(), C.byref(prm), arr, len(paths), None))
    return str(src)


def answers(db, queries, t):
    return Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences(queries, t))


def test_file_database_reserve(ka, ctx, oracle, tmp_path):
    from kwage_amd import native
    rng = np.random.default_rng(67)
    seqs = [li.random_dna(rng, 300) for _ in range(9)]
    accs = ["SRR%d" % (8300 + i) for i in range(9)]
    src = build_dbs(ka, ctx, oracle, tmp_path, seqs, accs, [("a.db", 10, range(0, 5)), ("b.db", 10, range(5, 9))])
    fresh = [li.random_dna(rng, 300) for _ in range(10)]
    queries = [seqs[1][10:150], seqs[6][50:250], seqs[4], fresh[0][30:200], fresh[8][:120], seqs[2][:60] + seqs[7][:60], li.random_dna(rng, 80)]
    db = ka.FileDatabase(ctx, [src], headroom=8)
    try:
        g = db.groups[0]
        assert len(db.groups) == 1 and g.room >= 8 and db.reserve(8) == [] and db.groups[0] is g
        for i in range(8):
            db.add_sample("SRR99990%02d" % i, [fresh[i]])
        # a row stride is a multiple of 128 bytes, so the group holds more than the headroom asked for: the rest of the row
        # is used up with empty filters (which no search reports) -- from here on the group is full
        if g.room:
            g.insert_filters(np.zeros((g.room, (1 << 10) // 8), dtype=np.uint8))
        assert g.room == 0
        with pytest.raises(native.KwageError, match="capacity exceeded"):
            db.add_sample("SRR9999008", [fresh[8]])
        before = {t: answers(db, queries, t) for t in (1.0, 0.7)}
        assert any(q == 3 and a == "SRR9999000" for q, a, _, _ in before[1.0]) and not any(q == 4 for q, _, _, _ in before[1.0])
        m = g.num_columns
        stats = db.reserve(64)
        wide = db.groups[0]
        assert len(stats) == 1 and stats[0]["columns"] == m and stats[0]["first_column"] == 0 and not g._h and wide is not g
        assert wide.num_columns == m and wide.room == 8 * wide.row_stride - m >= 64 and 8 * wide.row_stride >= (m + 127) // 128 * 128 + 64
        assert {t: answers(db, queries, t) for t in (1.0, 0.7)} == before
        assert db.add_sample("SRR9999008", [fresh[8]]) == (0, m)
        new_sample = Counter((q, a, f, n) for q, a, f, n in answers(db, queries, 1.0) if a == "SRR9999008")
        assert any(q == 4 and f == n for q, a, f, n in new_sample)
        after = {t: answers(db, queries, t) for t in (1.0, 0.7)}
        assert after[1.0] == before[1.0] + new_sample
        assert Counter({h: c for h, c in after[0.7].items() if h[1] != "SRR9999008"}) == before[0.7]
        assert db.reserve(64) == [] and db.groups[0] is wide
        # retire, compact, save and a reload still agree
        db.retire_sample(accs[2])
        db.retire_sample("SRR9999003")
        got = {t: answers(db, queries, t) for t in (1.0, 0.7)}
        assert not any(a in (accs[2], "SRR9999003") for _, a, _, _ in got[0.7])
        assert got[1.0] == Counter({h: c for h, c in after[1.0].items() if h[1] not in (accs[2], "SRR9999003")})
        db.compact()
        assert {t: answers(db, queries, t) for t in (1.0, 0.7)} == got
        written = db.save(str(tmp_path / "saved"))
        assert len(written) == 1
    finally:
        db.close()
    again = ka.FileDatabase(ctx, [str(tmp_path / "saved")])
    try:
        assert {t: answers(again, queries, t) for t in (1.0, 0.7)} == got
    finally:
        again.close()


def test_file_database_merge_groups(ka, ctx, oracle, tmp_path):
    rng = np.random.default_rng(61)
    seqs = [li.random_dna(rng, 300) for _ in range(9)]
    accs = ["SRR%d" % (8200 + i) for i in range(9)]
    src = build_dbs(ka, ctx, oracle, tmp_path, seqs, accs, [("a.db", 12, range(0, 5)), ("b.db", 10, range(5, 9))])
    fresh = [li.random_dna(rng, 300) for _ in range(3)]
    queries = [seqs[1][10:150], seqs[6][50:250], seqs[4], fresh[0][30:200], fresh[1][:120], seqs[2][:60] + seqs[7][:60], li.random_dna(rng, 80), fresh[2]]
    db = ka.FileDatabase(ctx, [src], headroom=64)
    try:
        assert [g.params.log_2_filter_len for g in db.groups] == [10, 12] and db.merge_groups() == 0 and len(db.groups) == 2
        db.add_sample("SRR9999001", [fresh[0]], group=1)
        db.add_sample("SRR9999002", [fresh[1]], group=0)
        assert db.retire_sample(accs[2])[0] == 1 and db.retire_sample(accs[6])[0] == 0
        db.fold(10)
        assert [g.params.log_2_filter_len for g in db.groups] == [10, 10]
        before = {t: answers(db, queries, t) for t in (1.0, 0.7)}
        order = [db._accession(path, c) for _, _, path, c in db._samples()]
        old = list(db.groups)
        capacity = sum(8 * g.row_stride for g in old)
        assert db.merge_groups() == 1 and len(db.groups) == 1 and not any(g._h for g in old)
        one = db.groups[0]
        assert one.num_columns == 9 - 2 + 2 and 8 * one.row_stride == capacity and db._retired == set()
        assert [db._accession(path, c) for _, _, path, c in db._samples()] == order
        assert {t: answers(db, queries, t) for t in (1.0, 0.7)} == before
        assert any(a == "SRR9999001" and f == n for _, a, f, n in before[1.0]) and any(a == "SRR9999002" and f == n for _, a, f, n in before[1.0])
        assert db.merge_groups() == 0
        # the merged group is a live group like any other
        assert db.add_sample("SRR9999003", [fresh[2]]) == (0, 9)
        db.retire_sample(accs[0])
        got = {t: answers(db, queries, t) for t in (1.0, 0.7)}
        assert any(q == 7 and a == "SRR9999003" and f == n for q, a, f, n in got[1.0]) and not any(a == accs[0] for _, a, _, _ in got[0.7])
        written = db.save(str(tmp_path / "saved"))
        assert [w.rsplit("_", 1)[1] for w in written] == ["0000.db"]          # one numbering
    finally:
        db.close()
    again = ka.FileDatabase(ctx, [str(tmp_path / "saved")])
    try:
        assert len(again.groups) == 1 and again.groups[0].num_columns == 9 - 3 + 3
        assert {t: answers(again, queries, t) for t in (1.0, 0.7)} == got
    finally:
        again.close()
