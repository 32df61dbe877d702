"""The union of columns (include/kwage_amd.h: kwage_group_union_columns; Group.union_columns, FileDatabase.union_samples,
`kwage_dbtool union` and `merge`): new columns of a RESIDENT group, each the OR of listed columns of a resident group, made
on the device.

The expected matrix is the model's (tests/union_model.py: numpy, none of the planners), never the code under test; the
expected state is also that of a TWIN that received insert_filters(OR of export_filters(members)); the expected meaning is
the oracle's filter of the members' sequences together and the oracle's search on the image.  Every comparison is exact
equality."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import group_model as gm
import union_model as um

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
GUARD = 0x5A5A5A5A5A5A5A5A
STAT_FIELDS = ("first_column", "sets", "members", "entries", "first_unit", "units", "bytes_written")


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


def call(g, op):
    """A building step of tests/union_model.py on a device group -> what the model returns for it."""
    if op.kind == "add_columns":
        return g.add_columns(op.image, op.nf)
    if op.kind == "insert":
        return g.insert_filters(op.filters)
    if op.kind == "retire":
        g.retire_columns(op.cols)
    elif op.kind == "set_bits":
        g.set_bits(op.rows, op.cols)
    elif op.kind == "compact":
        g.compact()
    else:
        assert op.kind == "finalize", op.kind
        g.finalize()
    return 0


def union_abi(dst, src, sets, timing=False):
    """kwage_group_union_columns through ctypes -> (status, first_column, stats)"""
    from kwage_amd import native
    first = C.c_uint64(GUARD)
    st = native.UnionStats(first_column=GUARD, units=GUARD, kernel_ms=-1.0)
    offsets = np.zeros(len(sets) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    columns = np.ascontiguousarray([c for s in sets for c in s] or [0], dtype=np.uint64)
    rc = native.lib().kwage_group_union_columns(dst._h, src._h, columns.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), len(sets),
                                                2 if timing else 0, C.byref(first), C.byref(st))
    return rc, first.value, st


def check_against_model(g, m, what):
    """Span, column count, row bytes, every row and -- a finalized group -- the valid mask (through
    kwage_group_column_bits: 0 on a dead column)."""
    assert (g.column_span, g.num_columns, g.row_bytes, g.row_stride) == (m.span, m.num_columns, m.span // 8, m.stride), what
    assert np.array_equal(g.real_columns(), m.real), what
    if m.span:
        rows = g.read_rows(np.arange(m.nrows))
        assert np.array_equal(rows, m.packed()), (what, np.argwhere(rows != m.packed())[:5])
        if m.finalized:
            g._column_bits = None
            assert np.array_equal(g.column_bits(), np.where(m.real, m.bits.sum(axis=0), 0).astype(np.uint32)), what


def or_of_exports(g, sets):
    """uint8 [n, filter bytes]: per set the OR of the members' exported filters."""
    return np.stack([np.bitwise_or.reduce(g.export_filters(list(s)), axis=0) for s in sets])


# ------------------------------------------------------------------------------------------------------------------
# the twin comparison over the case table
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_case(ka, ctx, case):
    L = case[0]
    ops, dst_name, caps, rng = um.case_ops(case)
    models = um.fresh_models(case, caps)
    groups = {name: ka.Group(ctx, um.K, um.NH, L, cap) for name, cap in caps.items()}
    twin = ka.Group(ctx, um.K, um.NH, L, caps[dst_name])      # the same steps as the destination
    try:
        for op in ops:
            want = models[op.on].apply(op)
            got = call(groups[op.on], op)
            assert op.kind == "compact" or got == want, (op, got, want)
            if op.on == dst_name:
                call(twin, op)
        sets = um.lists_of(rng, case[3], models["S"])
        dst, src, md, ms = groups[dst_name], groups["S"], models[dst_name], models["S"]
        same = dst is src
        check_against_model(dst, md, "before")
        src_state = gm.state_of(src, 1 << L)
        ors = or_of_exports(twin if same else src, sets)
        # the model's filters are the ORs of the exported members
        assert np.array_equal(gm.columns_of(ors, L), np.stack([ms.matrix[:, s].any(axis=1) for s in sets], axis=1))
        timing = len(sets) % 2 == 1
        rc, first, st = union_abi(dst, src, sets, timing)
        want = um.union(md, ms, sets)
        n = len(sets)
        assert rc == 0 and first == want, (rc, first, want)
        units = (first + n + 127) // 128 - first // 128
        want_stats = {"first_column": first, "sets": n, "members": sum(len(s) for s in sets), "entries": sum(len({c // 32 for c in s}) for s in sets),
                      "first_unit": first // 128, "units": units, "bytes_written": (1 << L) * units * 16}
        assert {f: getattr(st, f) for f in STAT_FIELDS} == want_stats, want_stats
        assert (st.kernel_ms > 0) if timing else (st.kernel_ms == 0), st.kernel_ms
        dst._inserted(first, n)                       # (the call went around the Python mirror)
        check_against_model(dst, md, "after")
        if not same:
            assert gm.same_state(gm.state_of(src, 1 << L), src_state)
            check_against_model(src, ms, "source")
            # the twin took the same columns as filters: the same place, the same state
            assert twin.insert_filters(ors) == first
            assert gm.same_state(gm.state_of(dst, 1 << L), gm.state_of(twin, 1 << L))
            if md.finalized:
                twin._column_bits = None
                assert np.array_equal(dst.column_bits(), twin.column_bits())
        else:
            # (the twin's insert continues at its open tail: another place, the same columns)
            t_first = twin.insert_filters(ors)
            assert t_first <= first
            assert np.array_equal(dst.export_filters(list(range(first, first + n))), twin.export_filters(list(range(t_first, t_first + n))))
        # a following insert lands right behind the union
        more = gm.Op("insert", on=dst_name, filters=gm.random_filters(rng, L, 3))
        assert call(dst, more) == md.apply(more) == first + n
        check_against_model(dst, md, "a following insert")
        if not md.finalized:                          # every byte of the row up to the stride
            for op in um.reveal_ops(md, dst_name):
                assert call(dst, op) == md.apply(op)
            check_against_model(dst, md, "to the stride")
            assert call(dst, gm.Op("finalize")) == md.finalize()
            check_against_model(dst, md, "finalized at last: the valid mask")
    finally:
        twin.close()
        for g in groups.values():
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# singletons: a union of one-member sets is the copy
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", [0, 33])
def test_singletons_are_the_copy(ka, ctx, tail):
    L, rng = 6, np.random.default_rng(17 + tail)
    src, a, b = (ka.Group(ctx, um.K, um.NH, L, 1400) for _ in range(3))
    try:
        src.add_columns(um._random_image(rng, 1 << L, 77), 77)
        src.insert_filters(gm.random_filters(rng, L, 300))
        src.retire_columns([130, 131, 200])
        valid = np.flatnonzero(src.real_columns())
        cols = [int(c) for c in rng.permutation(valid)[:150]]
        if tail:
            f = gm.random_filters(rng, L, tail)
            a.insert_filters(f)
            b.insert_filters(f)
        first, st = a.union_columns([[c] for c in cols], src)
        assert (first, st["sets"], st["members"], st["entries"]) == (tail, 150, 150, 150)
        assert b.copy_columns_from(src, cols)[0] == first
        assert gm.same_state(gm.state_of(a, 1 << L), gm.state_of(b, 1 << L))
        assert a.room == b.room
        a.finalize()
        b.finalize()
        assert np.array_equal(a.column_bits(), b.column_bits()) and a.column_bits()[first:first + 150].any()
    finally:
        for g in (src, a, b):
            g.close()


# ------------------------------------------------------------------------------------------------------------------
# the meaning: the union column is the filter of all the members' sequences together
# ------------------------------------------------------------------------------------------------------------------

def test_meaning_against_the_oracle(ka, ctx, oracle):
    k, nh, lg = 21, 3, 11
    rng = np.random.default_rng(29)
    A, B, Cs = ([gm.random_dna(rng, 150) for _ in range(2)] for _ in range(3))
    others = [[gm.random_dna(rng, 150)] for _ in range(4)]
    samples = [A, B, Cs] + others
    filters = np.stack([oracle.bloom_bits_from_sequences(s, k, nh, lg) for s in samples])
    together = oracle.bloom_bits_from_sequences(A + B + Cs, k, nh, lg)
    queries = [B[0][20:120], Cs[1][5:140], B[1][:60] + Cs[0][:60], A[0], others[1][0][10:100], gm.random_dna(rng, 80)]
    g = ka.Group(ctx, k, nh, lg, 512)
    try:
        assert g.insert_filters(filters) == 0
        g.finalize()
        first, st = g.union_columns([[0, 1, 2]])
        assert first == 128 and st["entries"] == 1
        assert np.array_equal(g.export_filters([first])[0], together)
        image = gm.Image(lg)
        image.put(0, gm.columns_of(filters, lg))
        image.put(first, gm.columns_of(together[None, :], lg))
        gm.check_rows(g, image)
        b = ka.Batch(ctx, queries)
        try:
            for t in (1.0, 0.8):
                exp = gm.oracle_hits(oracle, image, k, nh, lg, queries, t)
                for q in (0, 1, 3):                  # cut from B, cut from C, A whole: the union holds them all
                    assert (q, first) in {(h[0], h[1]) for h in exp}, (t, q)
                for flags in (0, ka.SEARCH_EARLY_EXIT):
                    assert [tuple(h) for h in g.search(b, t, flags).hits.tolist()] == exp, (t, flags)
        finally:
            b.close()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# the union commutes with the fold
# ------------------------------------------------------------------------------------------------------------------

def test_commutes_with_fold(ka, ctx):
    L, rng = 8, np.random.default_rng(31)
    g = ka.Group(ctx, um.K, um.NH, L, 1400)
    made = [g]
    try:
        g.insert_filters(gm.random_filters(rng, L, 90) & gm.random_filters(rng, L, 90) & gm.random_filters(rng, L, 90))
        g.retire_columns([40])
        valid = [c for c in range(90) if c != 40]
        sets = [[0, 1], valid, [39, 41, 89], [7]] + [[int(c) for c in rng.choice(valid, size=5)] for _ in range(140)]
        before, _ = g.fold(L - 2)
        made.append(before)
        first, _ = g.union_columns(sets)
        after, _ = g.fold(L - 2)
        made.append(after)
        first2, _ = before.union_columns(sets)
        assert first == first2 == 128
        new = list(range(first, first + len(sets)))
        got, want = after.export_filters(new), before.export_filters(new)
        assert np.array_equal(got, want) and got.any()
        assert gm.same_state(gm.state_of(after, 1 << (L - 2)), gm.state_of(before, 1 << (L - 2)))
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------------------------------------------------------
# refusals: in order, each found before a byte is written or allocated
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_in_order_change_nothing(ka, ctx):
    from kwage_amd import native
    lib = native.lib()
    L, nrows = 6, 64
    rng = np.random.default_rng(37)
    dst, src = ka.Group(ctx, um.K, um.NH, L, 1024), ka.Group(ctx, um.K, um.NH, L, 1024)
    sparse = ka.Group.sparse(ctx, um.K, um.NH, L, 1024, np.arange(0, nrows, 2))
    differing = [ka.Group(ctx, um.K + 2, um.NH, L, 256), ka.Group(ctx, um.K, um.NH + 1, L, 256), ka.Group(ctx, um.K, um.NH, L - 1, 256)]
    searched = ka.Group(ctx, um.K, um.NH, L, 256)
    other_ctx = ka.Context(0)
    foreign = ka.Group(other_ctx, um.K, um.NH, L, 256)
    b = ka.Batch(ctx, [gm.random_dna(rng, 30) for _ in range(8)])
    try:
        assert dst.insert_filters(gm.random_filters(rng, L, 37)) == 0
        src.add_columns(um._random_image(rng, nrows, 77), 77)
        src.insert_filters(gm.random_filters(rng, L, 40))     # columns 128 .. 167
        src.retire_columns([130])
        for g in differing + [searched, foreign]:
            g.insert_filters(gm.random_filters(rng, int(g.params.log_2_filter_len), 5))
        searched.finalize()
        searched.submit(b, 1.0).collect()           # (the context's search scratch exists from here on)
        ctx.sync()
        states = gm.state_of(dst, nrows), gm.state_of(src, nrows)
        free = ctx.mem_info()[0]

        def refused(rc_first_st, status, word):
            rc, first, st = rc_first_st
            assert rc == status and word in lib.kwage_last_error(), (rc, word, lib.kwage_last_error())
            assert first == GUARD and st.first_column == GUARD and st.units == GUARD and st.kernel_ms == -1.0
            assert gm.same_state(gm.state_of(dst, nrows), states[0]) and gm.same_state(gm.state_of(src, nrows), states[1])

        first = C.c_uint64(GUARD)
        cols = (C.c_uint64 * 3)(0, 1, 2)
        offs = (C.c_uint64 * 3)(0, 2, 3)
        f = C.byref(first)
        # every earlier refusal wins over every later one: each call carries all the later faults too
        for args, word in (((None, src._h, cols, offs, 2, 0, f, None), b"NULL dst"), ((dst._h, None, cols, offs, 2, 0, f, None), b"NULL src"),
                           ((dst._h, src._h, None, offs, 2, 0, f, None), b"NULL columns"), ((dst._h, src._h, cols, None, 2, 0, f, None), b"NULL set_offsets"),
                           ((dst._h, src._h, cols, offs, 0, 0, None, None), b"NULL first_column")):
            assert lib.kwage_group_union_columns(*args) == ERR_ARG and word in lib.kwage_last_error(), lib.kwage_last_error()
        bad0, down, empty = (C.c_uint64 * 3)(1, 2, 3), (C.c_uint64 * 3)(0, 2, 1), (C.c_uint64 * 3)(0, 2, 2)
        for o, n, word in ((bad0, 0, b"n_sets is 0"), (bad0, 2, b"set_offsets[0]"), (down, 2, b"decreases"), (empty, 2, b"is empty")):
            assert lib.kwage_group_union_columns(dst._h, foreign._h, cols, o, n, 0, f, None) == ERR_ARG and word in lib.kwage_last_error(), lib.kwage_last_error()
        assert first.value == GUARD
        beyond = [[0, 100000]]
        refused(union_abi(dst, foreign, beyond, True), ERR_ARG, b"different contexts")
        refused(union_abi(dst, sparse, beyond, True), ERR_ARG, b"sparse")
        refused(union_abi(sparse, src, beyond, True), ERR_ARG, b"sparse")
        for g, word in zip(differing, (b"kmer_len", b"num_hash", b"log_2_filter_len")):
            refused(union_abi(dst, g, beyond, True), ERR_ARG, word)
            refused(union_abi(g, dst, beyond, True), ERR_ARG, word)
        # (hash_func: kwage_group_create accepts one hash function only -- the refusal is tests/sanitize/union_sanitize.cpp's)
        pending = searched.submit(b, 1.0)
        out = union_abi(dst, src, beyond, True), union_abi(src, src, beyond, True)
        pending.collect()
        refused(out[0], ERR_STATE, b"pending")
        assert out[1][0] == ERR_STATE and out[1][1] == GUARD
        ctx.sync()
        too_many = [[0]] * (8 * dst.row_stride - 37 + 1)
        refused(union_abi(dst, src, [[0], [1, src.column_span]] + too_many, True), ERR_ARG, b"beyond the span")
        refused(union_abi(dst, src, [[0, 76], [77]] + too_many, True), ERR_ARG, b"pad or retired")          # (a file block's pad)
        refused(union_abi(dst, src, [[129, 130]] + too_many, True), ERR_ARG, b"pad or retired")            # (a retired column)
        refused(union_abi(src, src, [[0, 120]], True), ERR_ARG, b"pad or retired")                        # (between the blocks)
        refused(union_abi(dst, src, too_many, True), ERR_ARG, b"capacity exceeded")
        refused(union_abi(src, src, [[0]] * (8 * src.row_stride - 256 + 1), True), ERR_ARG, b"capacity exceeded")      # (behind the pad to column 256)
        assert ctx.mem_info()[0] == free
        # and the same calls succeed afterwards: up to the last column of the row, without stats too
        rc, got, st = union_abi(dst, src, [[0, 76], [129, 131], [0, 0]], True)
        assert rc == 0 and got == 37 and (st.sets, st.members, st.entries) == (3, 6, 4)
        fill = [[0]] * (8 * dst.row_stride - 40)
        o = np.arange(len(fill) + 1, dtype=np.uint64)
        c = np.zeros(len(fill), dtype=np.uint64)
        assert lib.kwage_group_union_columns(dst._h, src._h, c.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), len(fill), 0, f, None) == 0 and first.value == 40
        assert dst.column_span == 8 * dst.row_stride and gm.same_state(gm.state_of(src, nrows), states[1])
        assert np.array_equal(dst.export_filters([39, 40, 8 * dst.row_stride - 1]), src.export_filters([0, 0, 0]))
    finally:
        b.close()
        for g in [dst, src, sparse, searched, foreign] + differing:
            g.close()
        other_ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# FileDatabase.union_samples and the command line, on the golden `.db` files
# ------------------------------------------------------------------------------------------------------------------

def db_columns(oracle, path):
    """([run accession of column j], bool [2^L, num_filter]) of a `.db` file, read with the oracle's reader."""
    f = oracle.read_db(path)
    bits = np.unpackbits(np.asarray(f.rows), axis=1, bitorder="little")[:, :f.header.num_filter].astype(bool)
    return [oracle.accession_to_str(f.info(j).run_accession) for j in range(f.header.num_filter)], bits, f


def answers(db, queries, t):
    return Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences(queries, t))


def golden_unions(accs):
    return [("SRR9990001", [accs[3], accs[4], accs[50]]), ("SRR9990002", [accs[99]]), ("SRR9990003", [accs[4], accs[5], accs[4]])]


def check_union_file(oracle, out_db, in_db, unions, dropped):
    """The output file: per union one column, the OR of the members' columns of the input; every other column and its
    record as in the input, the members left out where they were dropped."""
    accs0, bits0, f0 = db_columns(oracle, in_db)
    accs1, bits1, f1 = db_columns(oracle, out_db)
    gone = {a for _, members in unions for a in members} if dropped else set()
    kept = [j for j, a in enumerate(accs0) if a not in gone]
    assert accs1 == [accs0[j] for j in kept] + [new for new, _ in unions]
    assert np.array_equal(bits1[:, :len(kept)], bits0[:, kept])
    for i, j in enumerate(kept):
        assert f1.info(i) == f0.info(j)
    for i, (new, members) in enumerate(unions):
        want = bits0[:, [accs0.index(a) for a in members]].any(axis=1)
        assert np.array_equal(bits1[:, len(kept) + i], want) and want.any(), new
        assert f1.info(len(kept) + i) == oracle.FilterInfo(run_accession=oracle.str_to_accession(new))
    return bits1[:, len(kept):]


@pytest.mark.parametrize("retire", [False, True])
def test_file_database_union_samples(ka, ctx, oracle, golden_dir, tmp_path, retire):
    src = os.path.join(golden_dir, "basic", "db")
    in_db = os.path.join(src, "basic.db")
    accs0, _, _ = db_columns(oracle, in_db)
    queries = [s for _, s in oracle.read_sequences(os.path.join(golden_dir, "basic", "q.fa"))][:12]
    unions = golden_unions(accs0)
    members = {a for _, ms in unions for a in ms}
    db = ka.FileDatabase(ctx, [src], headroom=256)
    try:
        before = {t: answers(db, queries, t) for t in (1.0, 0.5)}
        assert any(a in members for _, a, _, _ in before[0.5])
        with pytest.raises(KeyError):
            db.union_samples([("SRR9990009", [accs0[0], "SRR7777777"])])
        assert db.groups[0].num_columns == 100 and answers(db, queries, 0.5) == before[0.5]
        first = (db.groups[0].row_bytes + 15) // 16 * 16 * 8
        assert db.union_samples(unions, retire=retire) == [(0, first), (0, first + 1), (0, first + 2)]
        assert db.groups[0].num_columns == 103 - (5 if retire else 0)
        got = {t: answers(db, queries, t) for t in (1.0, 0.5)}
        for t in (1.0, 0.5):
            # whatever a member answered, its union answers with at least as many k-mers; everything else answers as before
            for q, a, f, n in before[t]:
                for new, ms in unions:
                    if a in ms:
                        assert any(q2 == q and a2 == new and f2 >= f and n2 == n for q2, a2, f2, n2 in got[t]), (t, q, a, new)
            old = Counter({h: c for h, c in got[t].items() if h[1] not in [new for new, _ in unions]})
            assert old == Counter({h: c for h, c in before[t].items() if not (retire and h[1] in members)})
        written = db.save(str(tmp_path / "saved"))
        assert len(written) == 1
    finally:
        db.close()
    check_union_file(oracle, written[0], in_db, [(new, list(dict.fromkeys(ms))) for new, ms in unions], retire)
    again = ka.FileDatabase(ctx, [str(tmp_path / "saved")])
    try:
        assert {t: answers(again, queries, t) for t in (1.0, 0.5)} == got
    finally:
        again.close()


def test_file_database_union_stays_within_one_group(ka, ctx, oracle, golden_dir):
    db = ka.FileDatabase(ctx, [os.path.join(golden_dir, "multi", "dbs")], headroom=256)
    try:
        assert len(db.groups) >= 2
        per_group = {}
        for gi, col, path, c in db._samples():
            per_group.setdefault(gi, db._accession(path, c))
        a, b = per_group[0], per_group[1]
        state = [(g.column_span, g.num_columns) for g in db.groups]
        with pytest.raises(ValueError, match="log_2_filter_len|kmer_len"):
            db.union_samples([("SRR9990001", [a]), ("SRR9990002", [a, b])])
        assert [(g.column_span, g.num_columns) for g in db.groups] == state
        # one call per group, one live block per group; a union sample is retired like any other
        out = db.union_samples([("SRR9990001", [a]), ("SRR9990002", [b]), ("SRR9990003", [a, a])])
        assert [gi for gi, _ in out] == [0, 1, 0] and out[2][1] == out[0][1] + 1
        assert db.retire_sample("SRR9990003") == out[2] and db.retire_sample("SRR9990001") == out[0]
        with pytest.raises(KeyError):
            db.retire_sample("SRR9990001")
        assert [db._accession(path, c) for _, _, path, c in db._samples()].count("SRR9990002") == 1
    finally:
        db.close()


@pytest.mark.parametrize("cmd", ["union", "merge"])
def test_dbtool_union_and_merge(ka, oracle, golden_dir, tmp_path, cmd):
    import math
    import re
    from kwage_amd import native
    tool = native.KWAGE_DBTOOL_BIN
    in_db = os.path.join(golden_dir, "basic", "db", "basic.db")
    accs0, bits0, f0 = db_columns(oracle, in_db)
    unions = golden_unions(accs0)

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    out_db = str(tmp_path / "out.db")
    r = run(cmd, out_db, in_db, *["%s=%s" % (new, ",".join(ms)) for new, ms in unions])
    assert r.returncode == 0, r.stderr
    new_bits = check_union_file(oracle, out_db, in_db, unions, cmd == "merge")
    nh, rows = f0.header.num_hash, float(bits0.shape[0])
    for i, (new, ms) in enumerate(unions):
        m = re.search(r"%s %s: (\d+) members, (\d+) bits set of (\d+) \(largest member (\d+)\), fill (\S+), false-positive rate (\S+)\n" % (cmd, new), r.stderr)
        assert m, r.stderr
        n = int(new_bits[:, i].sum())
        top = max(int(bits0[:, accs0.index(a)].sum()) for a in ms)
        assert m.groups() == (str(len(ms)), str(n), "%.0f" % rows, str(top), "%.6f" % (n / rows), "%.6g" % math.pow(n / rows, nh))
    # a member that is not in the file: exit code 1, nothing written; a malformed argument: the usage text, exit code 2
    nothing = str(tmp_path / "nothing.db")
    r = run(cmd, nothing, in_db, "SRR9990001=%s,SRR7777777" % accs0[0])
    assert r.returncode == 1 and "SRR7777777" in r.stderr and not os.path.exists(nothing)
    for bad in ("SRR9990001", "=%s" % accs0[0], "SRR9990001=", "SRR9990001=%s," % accs0[0]):
        r = run(cmd, nothing, in_db, bad)
        assert r.returncode == 2 and "usage" in r.stderr and not os.path.exists(nothing), bad
