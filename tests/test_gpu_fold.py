"""Fold (include/kwage_amd.h: kwage_group_fold; Group.fold, FileDatabase.fold, `kwage_dbtool fold`): a new group whose
Bloom filters are 2^L' bits long, made on the device from a RESIDENT group with longer ones.

Expected values are never the code under test's: the matrix is numpy's OR over the 2^f blocks of rows of the image,
img.reshape(2**f, 2**L2, cols).any(axis=0) packed LSB first; the MEANING is the oracle's -- the filters of the same
sequences built at the short length (kwage_oracle.bloom_bits_from_sequences), and its searches on the image made of them.
Every comparison is exact equality."""
import ctypes as C
import math
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import compact_cases as cc
import test_gpu_compact as tc
import test_gpu_live_insert as li

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6
GUARD = 0x5A5A5A5A5A5A5A50


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


def folded(img, L, L2):
    """bool [2^L2, cols]: row r' the OR of rows r' + j * 2^L2 of the image."""
    return img.reshape(1 << (L - L2), 1 << L2, img.shape[1]).any(axis=0)


def pack(img):
    return np.packbits(img, axis=1, bitorder="little")


def fold_abi(g, L2, timing=False, stats=True):
    """kwage_group_fold through ctypes -> (status, the handle word, stats)"""
    from kwage_amd import native
    out = C.c_void_p(GUARD)
    st = native.FoldStats(log_2_before=77, kernel_ms=-1.0)
    rc = native.lib().kwage_group_fold(g._h, L2, 2 if timing else 0, C.byref(out), C.byref(st) if stats else None)
    return rc, out, st


def plan(row_bytes, L, L2):
    """What kwage_fold_stats must report: the units of a row, and the bytes the items read and write."""
    units = (row_bytes + 15) // 16
    return {"log_2_before": L, "log_2_after": L2, "units_per_row": units, "bytes_read": (1 << L) * units * 16, "bytes_written": (1 << L2) * units * 16}


def native_lib():
    from kwage_amd import native
    return native.lib()


# ------------------------------------------------------------------------------------------------------------------
# 1. the matrix
# ------------------------------------------------------------------------------------------------------------------

PAIRS = [(1, 0), (3, 2), (3, 0), (8, 7), (8, 6), (8, 5), (8, 4), (8, 0), (12, 9)]
SPANS = [8, 120, 128, 136, 1016, 1024, 1032, 8200]


@pytest.mark.parametrize("L,L2", PAIRS, ids=lambda v: str(v))
def test_matrix(ka, ctx, L, L2):
    rng = np.random.default_rng(100 * L + L2)
    for span in SPANS:
        img = rng.random((1 << L, span)) < 1 / 16
        g = ka.Group(ctx, 21, 2, L, span)
        f = None
        try:
            assert g.add_columns(pack(img), span) == 0
            before = g.read_rows(np.arange(1 << L))
            f, st = g.fold(L2, timing=True)
            want = plan(g.row_bytes, L, L2)
            assert {k: st[k] for k in want} == want and st["kernel_ms"] > 0, st
            assert (f.column_span, f.row_bytes, f.num_columns, f.row_stride) == (g.column_span, g.row_bytes, g.num_columns, g.row_stride)
            assert f.params.log_2_filter_len == L2 and f.device_bytes == f.row_stride << L2
            got = f.read_rows(np.arange(1 << L2))
            exp = pack(folded(img, L, L2))
            assert np.array_equal(got, exp), (span, np.argwhere(got != exp)[:5])
            assert np.array_equal(g.read_rows(np.arange(1 << L)), before)
            image = li.Image(L2)
            image.put(0, folded(img, L, L2))
            li.check_zero_to_the_stride(ka, f, image)
        finally:
            g.close()
            if f is not None:
                f.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. layouts: file blocks, inserts at bit offsets, retired columns, bits planted in pad columns
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("finalized", [False, True], ids=["open", "finalized"])
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_layout(ka, ctx, case, finalized):
    L, L2 = 8, 5
    g, img, lay = tc.build(ka, ctx, case, L, finalized)
    rng = np.random.default_rng(len(lay.columns))
    f = None
    b = ka.Batch(ctx, [li.random_dna(rng, 40)])
    try:
        dead = np.flatnonzero(~lay.valid)
        if dead.size:                               # bits in pad and retired columns: folded like any others, masked as before
            rows, cols = rng.integers(0, 1 << L, size=6), rng.choice(dead, size=6)
            g.set_bits(rows, cols)
            img[rows, cols] = True
        before = li.state_of(g, 1 << L)
        f, st = g.fold(L2)
        assert li.same_state(li.state_of(g, 1 << L), before)
        assert (f.column_span, f.row_bytes, f.num_columns, f.row_stride) == (lay.span, lay.span // 8, lay.m, g.row_stride)
        assert np.array_equal(f.real_columns(), lay.valid) and np.array_equal(g.real_columns(), lay.valid)
        want = folded(img, L, L2)
        if lay.span:
            got = f.read_rows(np.arange(1 << L2))
            assert np.array_equal(got, pack(want)), np.argwhere(got != pack(want))[:5]
        # finalized as the source is: a search is refused before finalize
        for grp in (g, f):
            if finalized:
                assert all(lay.valid[c] for _, c, _ in grp.search(b, 1.0).hits.tolist())
            else:
                with pytest.raises(Exception) as e:
                    grp.search(b, 1.0)
                assert e.value.code == ERR_STATE
        # the next insert lands where the source's would
        n = 3
        fresh = rng.random((1 << L2, n)) < 0.5
        try:
            first = g.insert_filters(tc.filters_of(rng.random((1 << L, n)) < 0.5, list(range(n))))
        except Exception as e:
            first = None
            assert e.code == ERR_ARG
        if first is None:
            with pytest.raises(Exception) as e:
                f.insert_filters(tc.filters_of(fresh, list(range(n))))
            assert e.value.code == ERR_ARG
        else:
            assert first == (lay.tail if lay.tail is not None else (lay.span // 8 + 15) // 16 * 128)
            assert f.insert_filters(tc.filters_of(fresh, list(range(n)))) == first
            span = (first + n + 7) // 8 * 8
            exp = np.zeros((1 << L2, span), dtype=bool)
            exp[:, :lay.span] = want
            exp[:, first:first + n] = fresh
            exp[:, first + n:] = False              # (the insert owns its last word: zero at and above the new tail)
            assert f.column_span == span and f.num_columns == lay.m + n
            assert np.array_equal(f.read_rows(np.arange(1 << L2)), pack(exp))
    finally:
        b.close()
        g.close()
        if f is not None:
            f.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. the meaning, and every search on the folded group
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def samples():
    """40 sequences of 300 bases and queries drawn from them plus random ones (shared, never changed)."""
    rng = np.random.default_rng(31)
    seqs = [li.random_dna(rng, 300) for _ in range(40)]
    queries = [seqs[0][:80], seqs[7][100:260], seqs[39], seqs[3][10:40] + seqs[4][10:40], seqs[12][5:90], li.random_dna(rng, 60), li.random_dna(rng, 25),
               li.random_dna(rng, 21), li.random_dna(rng, 12)]
    return seqs, queries


@pytest.mark.parametrize("nh", [1, 3, 5])
def test_meaning_and_searches(ka, ctx, oracle, samples, nh):
    seqs, queries = samples
    k, L = 21, 12
    long = np.stack([oracle.bloom_bits_from_sequences([s], k, nh, L) for s in seqs])
    g = ka.Group(ctx, k, nh, L, 64)
    try:
        assert g.insert_filters(long) == 0
        g.finalize()
        for L2 in (10, 7):
            short = np.stack([oracle.bloom_bits_from_sequences([s], k, nh, L2) for s in seqs])
            f, _ = g.fold(L2)
            try:
                assert np.array_equal(f.export_filters(list(range(len(seqs)))), short)
                image = li.Image(L2)
                image.put(0, li.columns_of(short, L2))
                li.check_rows(f, image)
                b = ka.Batch(ctx, queries)
                try:
                    for t in (1.0, 0.6):
                        exp = li.oracle_hits(oracle, image, k, nh, L2, queries, t)
                        assert t < 1 or any(q == 2 and c == 39 for q, c, _ in exp)
                        for flags in (0, ka.SEARCH_EARLY_EXIT):
                            assert [tuple(h) for h in f.search(b, t, flags).hits.tolist()] == exp, (L2, t, flags)
                finally:
                    b.close()
                # top-k, scores, presence, column bits (and the threshold search at 0.8) against the oracle on the same image
                li.check_all_forms(ka, oracle, f, image, ctx, k, nh, L2, queries, [0, 39])
            finally:
                f.close()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. refusals and stats
# ------------------------------------------------------------------------------------------------------------------

def test_refusals_allocate_nothing(ka, ctx):
    from kwage_amd import native
    lib = native.lib()
    L = 8
    rng = np.random.default_rng(41)
    img = rng.random((1 << L, 200)) < 0.3
    g = ka.Group(ctx, 21, 2, L, 200)
    sparse = ka.Group.sparse(ctx, 21, 2, L, 200, np.arange(0, 1 << L, 2))
    b = ka.Batch(ctx, [li.random_dna(rng, 30) for _ in range(8)])
    try:
        assert g.add_columns(pack(img), 200) == 0
        g.finalize()
        g.submit(b, 1.0).collect()                  # (the context's search scratch exists from here on)
        ctx.sync()
        free = ctx.mem_info()[0]
        rc, out, st = fold_abi(sparse, 4)
        assert rc == ERR_ARG and b"sparse" in lib.kwage_last_error() and out.value == GUARD and st.log_2_before == 77
        for L2 in (L, L + 1):
            rc, out, st = fold_abi(g, L2)
            assert rc == ERR_ARG and b"not below" in lib.kwage_last_error() and out.value == GUARD and st.log_2_before == 77
        out = C.c_void_p(GUARD)
        assert lib.kwage_group_fold(None, 4, 0, C.byref(out), None) == ERR_ARG and b"NULL" in lib.kwage_last_error() and out.value == GUARD
        assert lib.kwage_group_fold(g._h, 4, 0, None, None) == ERR_ARG and b"NULL" in lib.kwage_last_error()
        pending = g.submit(b, 1.0)
        rc, out, st = fold_abi(g, 4)
        pending.collect()
        assert rc == ERR_STATE and b"pending" in lib.kwage_last_error() and out.value == GUARD and st.log_2_before == 77
        ctx.sync()
        assert ctx.mem_info()[0] == free
        # and the group still folds, without stats too
        rc, out, st = fold_abi(g, 4, stats=False)
        assert rc == 0 and out.value not in (None, GUARD)
        lib.kwage_group_destroy(out)
    finally:
        b.close()
        g.close()
        sparse.close()


def test_stats(ka, ctx):
    L = 9
    g = ka.Group(ctx, 21, 2, L, 3000)
    try:
        assert g.add_random_columns(1000, 5, 32) == 0 and g.add_random_columns(333, 6, 32) == 1024
        rb = g.row_bytes
        assert rb == 128 + 42
        for L2 in (8, 7, 6, 3):
            for timing in (True, False):
                rc, out, st = fold_abi(g, L2, timing=timing)
                assert rc == 0
                native_lib().kwage_group_destroy(out)
                want = plan(rb, L, L2)
                assert {k: getattr(st, k) for k in want} == want
                assert st.units_per_row == 11
                assert (st.kernel_ms > 0) if timing else (st.kernel_ms == 0), st.kernel_ms
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the command line and the files
# ------------------------------------------------------------------------------------------------------------------

def test_dbtool_fold(ka, ctx, oracle, tmp_path):
    from kwage_amd import native
    tool = native.KWAGE_DBTOOL_BIN
    k, nh, L, L2 = 21, 3, 12, 9
    rng = np.random.default_rng(51)
    seqs = [li.random_dna(rng, 300) for _ in range(3)]
    accs = ["SRR%d" % (8100 + i) for i in range(3)]

    def blooms(lg, where):
        where.mkdir()
        paths, bits = [], []
        for a, s in zip(accs, seqs):
            p = str(where / (a + ".bloom"))
            bits.append(oracle.bloom_bits_from_sequences([s], k, nh, lg))
            oracle.write_bloom(p, k, lg, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession(a), number_of_bases=300), bits[-1])
            paths.append(p)
        return paths, np.stack(bits)

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    long_paths, long_bits = blooms(L, tmp_path / "long")
    short_paths, short_bits = blooms(L2, tmp_path / "short")
    in_db, in_dbz = str(tmp_path / "in.db"), str(tmp_path / "in.dbz")
    r = run("build", in_db, str(k), str(L), str(nh), *long_paths)
    assert r.returncode == 0, r.stderr
    want = oracle.build_db_bytes(short_paths)
    got_dir, want_dir = tmp_path / "got", tmp_path / "want"
    got_dir.mkdir()
    want_dir.mkdir()
    (want_dir / "out.db").write_bytes(want)
    out_db = str(got_dir / "out.db")
    r = run("fold", out_db, in_db, str(L2))
    assert r.returncode == 0, r.stderr
    assert open(out_db, "rb").read() == want
    queries = [seqs[0][20:120], seqs[2], seqs[1][:50] + seqs[2][:50], li.random_dna(rng, 70)]
    for t in (1.0, 0.6):
        a, b = oracle.run_search([str(got_dir)], [], queries, t), oracle.run_search([str(want_dir)], [], queries, t)
        assert a == b and (t < 1 or "command line seq 1" in a)
    # the stderr line: shares of set bits per column before and after, from numpy
    m = re.search(r"fold 2\^12 -> 2\^9: set bits per column mean (\S+) largest (\S+) -> mean (\S+) largest (\S+), "
                  r"false-positive rate of the largest (\S+) -> (\S+),", r.stderr)
    assert m, r.stderr
    shares = []
    for bits, lg in ((long_bits, L), (short_bits, L2)):
        counts = np.unpackbits(bits, axis=1, bitorder="little").sum(axis=1)
        shares.append((float(counts.sum()) / float(1 << lg) / 3.0, float(counts.max()) / float(1 << lg)))
    assert m.groups() == ("%.6f" % shares[0][0], "%.6f" % shares[0][1], "%.6f" % shares[1][0], "%.6f" % shares[1][1],
                          "%.6g" % math.pow(shares[0][1], nh), "%.6g" % math.pow(shares[1][1], nh))
    # a compressed input gives the same bytes
    r = run("compress", in_db, in_dbz)
    assert r.returncode == 0, r.stderr
    out2 = str(tmp_path / "out2.db")
    r = run("fold", out2, in_dbz, str(L2))
    assert r.returncode == 0, r.stderr
    assert open(out2, "rb").read() == want
    # a length not below the file's: exit code 1, nothing written
    for lg in (L, L + 1):
        nothing = str(tmp_path / ("nothing%d.db" % lg))
        r = run("fold", nothing, in_db, str(lg))
        assert r.returncode == 1 and "not below" in r.stderr and not os.path.exists(nothing)


def test_file_database_fold(ka, ctx, oracle, tmp_path):
    from kwage_amd.native import lib, check, Params
    k, nh = 21, 2
    rng = np.random.default_rng(61)
    seqs = [li.random_dna(rng, 300) for _ in range(9)]
    accs = ["SRR%d" % (8200 + i) for i in range(9)]
    src = tmp_path / "src"
    src.mkdir()

    def build(name, lg, members):
        paths = []
        for i in members:
            p = str(tmp_path / ("%s_L%d.bloom" % (accs[i], lg)))
            oracle.write_bloom(p, k, lg, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession(accs[i])), oracle.bloom_bits_from_sequences([seqs[i]], k, nh, lg))
            paths.append(p)
        prm = Params(k, nh, lg, 0)
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        check(lib().kwage_build_db(ctx._h, str(src / name).encode(), C.byref(prm), arr, len(paths), None))

    build("a.db", 12, range(0, 5))                  # folded to 10
    build("b.db", 10, range(5, 9))                  # already there: left alone, and still a group of its own
    fresh = [li.random_dna(rng, 300) for _ in range(2)]
    queries = [seqs[1][10:150], seqs[6][50:250], seqs[4], fresh[0][30:200], fresh[1][:120], seqs[2][:60] + seqs[7][:60], li.random_dna(rng, 80)]

    def answers(db, t):
        return Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences(queries, t))

    db = ka.FileDatabase(ctx, [str(src)], headroom=64)
    try:
        assert [g.params.log_2_filter_len for g in db.groups] == [10, 12]
        gi, col = db.add_sample("SRR9999001", [fresh[0]], group=1)
        assert db.retire_sample(accs[2])[0] == 1
        spans = [(g.column_span, g.num_columns, g.row_stride) for g in db.groups]
        old = db.groups[1]
        stats = db.fold(10)
        assert len(stats) == 1 and stats[0]["log_2_before"] == 12 and stats[0]["log_2_after"] == 10 and not old._h
        assert [g.params.log_2_filter_len for g in db.groups] == [10, 10] and len(db.groups) == 2
        assert [(g.column_span, g.num_columns, g.row_stride) for g in db.groups] == spans
        assert db.fold(10) == []
        # the same answers as the oracle's filters at the short length give: the folded sample is found whole
        got = {t: answers(db, t) for t in (1.0, 0.7)}
        assert any(a == "SRR9999001" and f == n for _, a, f, n in got[1.0]) and not any(a == accs[2] for _, a, _, _ in got[0.7])
        assert any(a == accs[1] and f == n for q, a, f, n in got[1.0] if q == 0)
        # add_sample hashes at the new length: found by its own sequence, right behind the first live sample
        assert db.add_sample("SRR9999002", [fresh[1]], group=1) == (1, col + 1)
        got = {t: answers(db, t) for t in (1.0, 0.7)}
        assert any(q == 4 and a == "SRR9999002" and f == n for q, a, f, n in got[1.0])
        assert db.retire_sample(accs[0])[0] == 1
        got = {t: answers(db, t) for t in (1.0, 0.7)}
        written = db.save(str(tmp_path / "saved"))
        assert len(written) == 2 and len(set(written)) == 2
        db.compact()
        assert {t: answers(db, t) for t in (1.0, 0.7)} == got
    finally:
        db.close()
    again = ka.FileDatabase(ctx, [str(tmp_path / "saved")])
    try:
        assert len(again.groups) == 1 and again.groups[0].params.log_2_filter_len == 10 and again.groups[0].num_columns == 9 - 2 + 2
        assert {t: answers(again, t) for t in (1.0, 0.7)} == got
    finally:
        again.close()
