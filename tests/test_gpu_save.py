"""Save (include/kwage_amd.h: kwage_group_save_db; Group.save_db, FileDatabase.save, `kwage_dbtool append` / `drop`): chosen
columns of a RESIDENT group written as one raw `.db` file, gathered and packed on the device.

Every comparison is of whole files, byte for byte, and the expected bytes are the oracle's, never the code under test:
kwage_oracle.build_db_bytes over the `.bloom` files of the columns saved, in the order saved (the filters come into the
group through insert_bloom_files), or kwage_oracle.read_db + numpy + write_db for columns that came from files.  The cases
are data: tests/save_cases.py.  Each call goes through the C ABI and through the Python mirror."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN

import save_cases as sc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -6


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


@pytest.fixture(scope="module")
def blooms(oracle, tmp_path_factory):
    """blooms(k, nh, L, n) -> paths of n `.bloom` files with random bits and run accession SRR<j + 1>: written once per
    parameter set and never changed (a longer request extends the set)."""
    made = {}

    def get(k, nh, L, n):
        key = (k, nh, L)
        if key not in made:
            made[key] = (str(tmp_path_factory.mktemp("blooms_k%d_h%d_L%d" % key)), [])
        d, paths = made[key]
        rng = np.random.default_rng([k, nh, L, len(paths)])
        while len(paths) < n:
            j = len(paths)
            p = os.path.join(d, "f%05d.bloom" % j)
            bits = rng.integers(0, 256, size=max(1, (1 << L) // 8), dtype=np.uint8)
            oracle.write_bloom(p, k, L, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (j + 1))), bits)
            paths.append(p)
        return paths[:n]
    return get


def live_source(j):
    return {"run_accession": "SRR%d" % (j + 1)}


def save_abi(g, out, columns, sources, staging=0):
    """kwage_group_save_db through ctypes -> (status, kwage_save_stats)"""
    from kwage_amd import native
    n = len(columns)
    arr = (native.SaveColumn * max(n, 1))()
    keep = []
    for i, (c, s) in enumerate(zip(columns, sources)):
        arr[i].column = c
        if isinstance(s, dict):
            si = native.SampleInfo(run_accession=s["run_accession"].encode())
            keep.append(si)
            arr[i].info = C.pointer(si)
        elif s is not None:
            arr[i].source_db, arr[i].source_column = s[0].encode(), s[1]
    st = native.SaveStats()
    return native.lib().kwage_group_save_db(g._h, out.encode(), arr, n, staging, C.byref(st)), st


def saved_both_ways(g, tmp_path, columns, sources, staging=0):
    """The file through the C ABI and through Group.save_db: the two must agree; -> (bytes, stats of the ABI call)"""
    a, b = str(tmp_path / "abi.db"), str(tmp_path / "py.db")
    rc, st = save_abi(g, a, columns, sources, staging)
    assert rc == 0, rc
    d = g.save_db(b, columns, sources, staging)
    raw = open(a, "rb").read()
    assert open(b, "rb").read() == raw
    assert d["db_bytes"] == st.db_bytes == len(raw) and d["runs"] == st.runs and d["chunks"] == st.chunks and st.extract_kernel_ms > 0
    assert sorted(os.listdir(str(tmp_path))) == ["abi.db", "py.db"]           # no temporary file is left
    os.remove(a)
    os.remove(b)
    return raw, st


def group_of(ka, ctx, blooms, case, finalize=True):
    """The case's group, the paths of its filters and the filters listed for the save."""
    n = sum(case["calls"])
    paths = blooms(sc.K, sc.NH, case["L"], n)
    g = ka.Group(ctx, sc.K, sc.NH, case["L"], n + 200)
    at = 0
    for c in case["calls"]:
        assert g.insert_bloom_files(paths[at:at + c]) == at
        at += c
    if case["retire"]:
        g.retire_columns(case["retire"])
    if finalize:
        g.finalize()
    return g, paths, sc.survivors(case)


def first_difference(got, want):
    if len(got) != len(want):
        return "length %d, expected %d" % (len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    return "first difference at byte %s of %d" % (np.flatnonzero(a != b)[:1].tolist(), len(want))


# ------------------------------------------------------------------------------------------------------------------
# 1-4, 6, 7: inserted filters, retired ones, reordered lists, wide rows
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case(ka, ctx, oracle, blooms, tmp_path, name):
    case = sc.CASES[name]
    g, paths, keep = group_of(ka, ctx, blooms, case)
    try:
        want = oracle.build_db_bytes([paths[j] for j in keep])
        got, st = saved_both_ways(g, tmp_path, keep, [live_source(j) for j in keep])
        assert got == want, first_difference(got, want)
        assert st.runs == sc.count_runs(keep) and (case["runs"] is None or st.runs == case["runs"]) and st.chunks == 1
        h = oracle.DBHeader.unpack(got)
        assert h.num_filter == len(keep) and h.compression == 0 and len(got) == st.db_bytes
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. file blocks with live columns behind
# ------------------------------------------------------------------------------------------------------------------

def test_file_blocks_with_live_columns_behind(ka, ctx, oracle, blooms, tmp_path):
    from kwage_amd.native import lib, check
    files = [os.path.join(GOLDEN, "multi", "dbs", "a", "k31_L10_h1.db"), os.path.join(GOLDEN, "multi", "dbs", "a", "deeper", "k31_L10_h1_b.db")]
    dbs = [oracle.read_db(f) for f in files]
    h0 = dbs[0].header
    k, nh, L = h0.kmer_len, h0.num_hash, h0.log_2_filter_len
    assert (k, nh, L) == (31, 1, 10) and all((d.header.kmer_len, d.header.num_hash, d.header.log_2_filter_len) == (k, nh, L) for d in dbs)
    live = blooms(k, nh, L, 5)
    g = ka.Group(ctx, k, nh, L, 4096)
    try:
        placed = g.add_db_files(files)
        assert placed[1][0] % 128 == 0 and placed[1][0] > placed[0][0] + placed[0][1]          # a 16-byte boundary, pad columns in between
        first = g.insert_bloom_files(live)
        assert first % 128 == 0 and first >= placed[1][0] + placed[1][1]
        g.finalize()
        # the expected file: the files' own columns and records, then the live filters'
        file_bits = [np.unpackbits(d.rows, axis=1, bitorder="little")[:, :d.header.num_filter] for d in dbs]
        file_infos = [[d.info(j) for j in range(d.header.num_filter)] for d in dbs]
        live_bits = np.stack([np.unpackbits(oracle.read_bloom(p)[3], bitorder="little")[:1 << L] for p in live], axis=1)
        live_infos = [oracle.read_bloom(p)[2] for p in live]
        file_cols = [(first_c + j, (f, j)) for (first_c, nf), f in zip(placed, files) for j in range(nf)]
        live_cols = [(first + j, live_source(j)) for j in range(5)]

        def expected(bits, infos):
            n = sum(b.shape[1] for b in bits)
            rows = np.packbits(np.concatenate(bits, axis=1), axis=1, bitorder="little")
            p = str(tmp_path / "expected.db")
            oracle.write_db(p, k, nh, L, rows, n, [i for part in infos for i in part])
            raw = open(p, "rb").read()
            os.remove(p)
            return raw

        for what, cols, bits, infos in (("all", file_cols + live_cols, file_bits + [live_bits], file_infos + [live_infos]),
                                        ("files", file_cols, file_bits, file_infos),
                                        ("live", live_cols, [live_bits], [live_infos])):
            want = expected(bits, infos)
            got, st = saved_both_ways(g, tmp_path, [c for c, _ in cols], [s for _, s in cols])
            assert got == want, (what, first_difference(got, want))
            assert st.runs == {"all": 3, "files": 2, "live": 1}[what]
            if what == "files":           # and what the re-pack makes of the two files
                rp = str(tmp_path / "repacked.db")
                arr = (C.c_char_p * 2)(*[f.encode() for f in files])
                check(lib().kwage_repack_db(ctx._h, rp.encode(), arr, 2))
                assert open(rp, "rb").read() == got
                os.remove(rp)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 8. staged chunks
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.STAGED))
def test_staged_chunks(ka, ctx, oracle, blooms, tmp_path, name):
    case_name, staging, chunks = sc.STAGED[name]
    g, paths, keep = group_of(ka, ctx, blooms, sc.CASES[case_name])
    try:
        want = oracle.build_db_bytes([paths[j] for j in keep])
        got, st = saved_both_ways(g, tmp_path, keep, [live_source(j) for j in keep], staging)
        assert st.chunks == chunks
        assert got == want, first_difference(got, want)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 9. the group is only read
# ------------------------------------------------------------------------------------------------------------------

def test_group_state(ka, ctx, oracle, blooms, tmp_path):
    case = sc.CASES["retired"]
    g, paths, keep = group_of(ka, ctx, blooms, case, finalize=False)
    rng = np.random.default_rng(9)
    queries = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(sc.K, sc.K + 3, size=24)]
    rows = np.arange(1 << case["L"])
    try:
        want = oracle.build_db_bytes([paths[j] for j in keep])
        sources = [live_source(j) for j in keep]

        def state():
            return g.num_columns, g.column_span, g.row_bytes, g.read_rows(rows)

        before = state()
        got, _ = saved_both_ways(g, tmp_path, keep, sources)           # not finalized yet
        assert got == want, first_difference(got, want)
        after = state()
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3])
        g.finalize()
        b = ka.Batch(ctx, queries)
        try:
            hits = {t: g.search(b, t, ka.SEARCH_EARLY_EXIT).hits.tolist() for t in (1.0, 0.8)}
            assert hits[1.0] and all(c in keep for _, c, _ in hits[1.0])
            got, _ = saved_both_ways(g, tmp_path, keep, sources)       # finalized: the same bytes
            assert got == want, first_difference(got, want)
            after = state()
            assert before[:3] == after[:3] and np.array_equal(before[3], after[3])
            assert not any(ctx.scratch_nonzero().values())
            assert {t: g.search(b, t, ka.SEARCH_EARLY_EXIT).hits.tolist() for t in (1.0, 0.8)} == hits
        finally:
            b.close()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------
# 10. refusals touch nothing
# ------------------------------------------------------------------------------------------------------------------

def test_refusals(ka, ctx, oracle, blooms, tmp_path):
    from kwage_amd.native import lib
    L = 10
    paths = blooms(sc.K, sc.NH, L, 20)
    rng = np.random.default_rng(10)
    g = ka.Group(ctx, sc.K, sc.NH, L, 300)
    sparse = ka.Group.sparse(ctx, sc.K, sc.NH, L, 300, np.arange(0, 1 << L, 2))
    out = str(tmp_path / "out.db")
    try:
        assert g.insert_bloom_files(paths) == 0
        g.retire_columns([3])
        g.finalize()
        assert g.column_span == 24 and g.num_columns == 19
        good = [j for j in range(20) if j != 3]
        src = [live_source(j) for j in good]
        meta = str(tmp_path / "meta.db")                                # a file to take records from: 19 columns
        assert save_abi(g, meta, good, src)[0] == 0
        kept = open(meta, "rb").read()
        assert kept == oracle.build_db_bytes([paths[j] for j in good])

        def refused(columns, sources, want=ERR_ARG, word=None):
            for target in (out, meta):                                  # a fresh path, and over an existing file
                rc, st = save_abi(g, target, columns, sources)
                assert rc == want, (rc, lib().kwage_last_error())
                assert word is None or word in lib().kwage_last_error(), lib().kwage_last_error()
                assert sorted(os.listdir(str(tmp_path))) == ["meta.db"] and open(meta, "rb").read() == kept

        refused([0, 3], [live_source(0), live_source(3)], word=b"retired")          # a retired column
        refused([0, 20], [live_source(0), live_source(20)], word=b"pad")            # a pad column of the last byte
        refused([0, 24], [live_source(0), live_source(24)], word=b"span")           # at the span
        refused([0, 1 << 40], [live_source(0), live_source(1)], word=b"span")
        refused([0, 5, 0], [live_source(0), live_source(5), live_source(0)], word=b"twice")
        refused([], [], word=b"n is 0")
        refused([0, 1], [live_source(0), None], word=b"neither")                    # an entry without source or info
        refused([0, 1], [(meta, 0), (meta, 19)], word=b"no column 19")              # source_column beyond its file
        refused([0, 1], [(meta, 0), (str(tmp_path / "missing.db"), 0)], want=-3)    # unreadable metadata
        refused([0], [{"run_accession": "X1"}])                                     # not an accession
        img = np.ascontiguousarray(rng.integers(0, 256, size=(1 << (L - 1), 3), dtype=np.uint8))
        assert sparse.add_columns(img, 24) == 0
        rc, _ = save_abi(sparse, out, [0, 1], [live_source(0), live_source(1)])
        assert rc == ERR_ARG and b"sparse" in lib().kwage_last_error() and not os.path.exists(out)
        # a pending search
        b = ka.Batch(ctx, ["".join(rng.choice(list("ACGT"), size=30)) for _ in range(8)])
        try:
            pending = g.submit(b, 1.0)
            rc, _ = save_abi(g, out, good, src)
            rc2, _ = save_abi(g, meta, good, src)
            pending.collect()
            assert (rc, rc2) == (ERR_STATE, ERR_STATE) and b"pending" in lib().kwage_last_error()
            assert sorted(os.listdir(str(tmp_path))) == ["meta.db"] and open(meta, "rb").read() == kept
        finally:
            b.close()
        # and the group still saves: over one of its own sources of metadata, records copied verbatim
        rc, st = save_abi(g, meta, good[::-1], [(meta, i) for i in range(19)][::-1])
        assert rc == 0 and open(meta, "rb").read() == oracle.build_db_bytes([paths[j] for j in good[::-1]])
        assert sorted(os.listdir(str(tmp_path))) == ["meta.db"]
    finally:
        g.close()
        sparse.close()


# ------------------------------------------------------------------------------------------------------------------
# 11. FileDatabase: save, reload, the same answers
# ------------------------------------------------------------------------------------------------------------------

def test_file_database_round_trip(ka, ctx, oracle, tmp_path):
    dbs = os.path.join(GOLDEN, "multi", "dbs")
    rng = np.random.default_rng(11)
    fresh = ["".join(rng.choice(list("ACGT"), size=400)) for _ in range(2)]
    reads = [s for _, s in oracle.read_sequences(os.path.join(GOLDEN, "multi", "reads.fastq"))][:12]
    queries = reads + [fresh[0][30:200], fresh[1][100:300], fresh[0][:60] + fresh[1][:60]]
    out_dir = str(tmp_path / "saved")
    db = ka.FileDatabase(ctx, [dbs], headroom=64)
    try:
        # what the saved files must hold, from the oracle's reading of the golden files: per group the accessions in file
        # order, the first sample of the first file gone, one live sample behind group 0's
        per_group = {}
        for f in db.files:
            d = oracle.read_db(f)
            key = (d.header.kmer_len, d.header.num_hash, d.header.log_2_filter_len, d.header.hash_func)
            per_group.setdefault(key, []).extend(d.info(j).csv_string() for j in range(d.header.num_filter))
        keys = sorted(per_group)
        victim = oracle.read_db(db.files[0]).info(0).csv_string()
        first_key = tuple(getattr(oracle.read_db(db.files[0]).header, n) for n in ("kmer_len", "num_hash", "log_2_filter_len", "hash_func"))
        assert db.add_sample("SRR9999001", [fresh[0]])[0] == 0
        assert db.add_sample("SRR9999002", [fresh[1]])[0] == 0
        db.retire_sample(victim)
        db.retire_sample("SRR9999001")
        per_group[first_key].remove(victim)
        per_group[keys[0]].append("SRR9999002")
        want = {t: Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences(queries, t)) for t in (1.0, 0.8)}
        assert any(a == "SRR9999002" for _, a, _, _ in want[1.0]) and not any(a in ("SRR9999001",) for _, a, _, _ in want[0.8])
        written = db.save(out_dir, max_columns=16)
    finally:
        db.close()
    # the files, read by the oracle: at most 16 columns each, group by group in order
    assert sorted(written) == sorted(os.path.join(out_dir, f) for f in os.listdir(out_dir))
    at = 0
    for key in keys:
        accs = per_group[key]
        for i in range(0, len(accs), 16):
            d = oracle.read_db(written[at])
            at += 1
            assert (d.header.kmer_len, d.header.num_hash, d.header.log_2_filter_len, d.header.hash_func) == key and d.header.compression == 0
            assert d.header.num_filter == len(accs[i:i + 16]) and [d.info(j).csv_string() for j in range(d.header.num_filter)] == accs[i:i + 16]
    assert at == len(written) and len(written) > len(keys)              # several files per group
    again = ka.FileDatabase(ctx, [out_dir])
    try:
        assert sum(g.num_columns for g in again.groups) == sum(len(a) for a in per_group.values())
        for t in (1.0, 0.8):
            got = Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in again.search_sequences(queries, t))
            assert got == want[t], t
    finally:
        again.close()
    if os.access(oracle.REF_KWAGE, os.X_OK):                            # the reference reads what was saved
        q = tmp_path / "q.fa"
        q.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(queries)))
        r = subprocess.run([oracle.REF_KWAGE, "-d", out_dir, "-i", str(q), "--o.csv", "-t", "1.0"], capture_output=True, text=True,
                           env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        ref = Counter((int(name[1:]), acc, found, nk) for name, recs in oracle.parse_csv(r.stdout).items() for acc, nk, found, _ in recs)
        assert ref == want[1.0]


# ------------------------------------------------------------------------------------------------------------------
# 12. kwage_dbtool append / drop
# ------------------------------------------------------------------------------------------------------------------

def test_dbtool_append_and_drop(ka, oracle, tmp_path):
    from kwage_amd import native
    tool = native.KWAGE_DBTOOL_BIN
    golden = os.path.join(GOLDEN, "k32")
    paths = [os.path.join(golden, "bloom", "f%06d.bloom" % i) for i in range(8)]
    (k, lg, nh, _), _, _, _ = oracle.read_bloom(paths[0])
    whole = open(os.path.join(golden, "k32.db"), "rb").read()
    five, eight, seven = str(tmp_path / "five.db"), str(tmp_path / "eight.db"), str(tmp_path / "seven.db")

    def run(*args):
        return subprocess.run([tool] + list(args), capture_output=True, text=True, timeout=120)

    r = run("build", five, str(k), str(lg), str(nh), *paths[:5])
    assert r.returncode == 0, r.stderr
    r = run("append", eight, five, *paths[5:])
    assert r.returncode == 0, r.stderr
    got = open(eight, "rb").read()
    assert got == whole, first_difference(got, whole)
    accs = [oracle.read_db(eight).info(j).csv_string() for j in range(8)]
    assert "SRR3" in accs
    r = run("drop", seven, eight, "SRR3")
    assert r.returncode == 0, r.stderr
    got = open(seven, "rb").read()
    want = oracle.build_db_bytes([p for p, a in zip(paths, accs) if a != "SRR3"])
    assert got == want, first_difference(got, want)
    r = run("drop", str(tmp_path / "never.db"), eight, "SRR4", "SRR77")
    assert r.returncode == 1 and "SRR77" in r.stderr and not os.path.exists(str(tmp_path / "never.db"))
    assert run("nonsense", "x").returncode == 2
    assert sorted(os.listdir(str(tmp_path))) == ["eight.db", "five.db", "seven.db"]
