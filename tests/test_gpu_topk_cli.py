"""kwage_top on the reference-written fixtures of tests/golden (basic, multi, k32): for t > 0 each query's rows are the
first K rows `kwage -t t` prints for it -- the same scores in the same order, the same samples except within a run of
equal scores that straddles row K.  A multi-file database gives what one repacked file gives, and
FileDatabase.search_sequences_top agrees with the program."""
import csv
import io
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = {
    "basic": (["-d", "db", "-i", "q.fa"],
              ["CGGTGTATGTCTTAGTAAATTGTTCAGGACAACTTGTACCCTACTAGGAGGCAGCCGTGTTTGTAAGGCTATTTTGACGTACCGTACTAACATAGCGGCT", "ACGTNACGT"]),
    "multi": (["-d", "dbs", "-i", "reads.fastq", "-i", "contigs.fa.gz"], []),
    "k32": (["-d", "k32.db", "-i", "q.fna"], []),
}


@pytest.fixture(scope="module")
def native():
    from kwage_amd import native
    native.ensure_built()
    return native


def _run(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=cwd, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode("latin-1")


def _rows(text, fmt):
    """{query: [(score, num_kmers, sample), ...]} in printed order."""
    out = {}
    if fmt == "csv":
        for rec in list(csv.reader(io.StringIO(text)))[1:]:
            out.setdefault(rec[0], []).append((int(rec[2]), int(rec[1]), rec[4]))
        return out
    doc = json.loads(text) if text.strip() else []
    for q in (doc if isinstance(doc, list) else [doc]):
        out[q["query"]] = [(r["num_kmers_found"], r["num_kmers"], json.dumps(r["sample_metadata"], sort_keys=True)) for r in q["results"]]
    return out


def _check_prefix(top, full, K, where):
    assert list(top) == list(full), where                  # the same queries, in the same order
    for q, rows in top.items():
        ref = full[q][:K]
        assert [r[:2] for r in rows] == [r[:2] for r in ref], (where, q)
        cut = ref[-1][0]
        straddles = len(full[q]) > K and full[q][K][0] == cut
        for s in {r[0] for r in ref}:
            mine = sorted(r[2] for r in rows if r[0] == s)
            theirs = sorted(r[2] for r in ref if r[0] == s)
            if s == cut and straddles:
                assert set(mine) <= {r[2] for r in full[q] if r[0] == s}, (where, q, s)
            else:
                assert mine == theirs, (where, q, s)


@pytest.mark.parametrize("case", sorted(CASES))
def test_kwage_top_is_a_prefix_of_kwage(native, case):
    args, seqs = CASES[case]
    cdir = os.path.join(GOLDEN, case)
    for t in ("1", "0.8", "0.5"):
        for fmt in ("csv", "json"):
            full = _rows(_run(native.KWAGE_BIN, args + ["-t", t, "--o." + fmt] + seqs, cdir), fmt)
            for K in (1, 3, 10, 1024):
                text = _run(native.KWAGE_TOP_BIN, args + ["-k", str(K), "-t", t, "--o." + fmt] + seqs, cdir)
                if fmt == "json" and text.strip():
                    assert ('"threshold": %.1f' % float(t)) in text
                _check_prefix(_rows(text, fmt), full, K, (case, t, fmt, K))


def test_kwage_top_threshold_zero_returns_k_rows(native):
    args, seqs = CASES["basic"]
    text = _run(native.KWAGE_TOP_BIN, args + ["-k", "7", "--o.csv"] + seqs, os.path.join(GOLDEN, "basic"))
    rows = _rows(text, "csv")
    assert rows and all(len(v) == 7 for v in rows.values())          # 100 samples: every query with k-mers fills k rows
    assert "command line seq 1" not in rows                          # "ACGTNACGT": no k-mers, no rows
    for v in rows.values():
        assert [r[0] for r in v] == sorted((r[0] for r in v), reverse=True)


def test_multi_file_database_equals_repacked_file(native, tmp_path):
    cdir = os.path.join(GOLDEN, "multi")
    files = [os.path.join(cdir, "dbs", "a", "k31_L10_h1.db"), os.path.join(cdir, "dbs", "a", "deeper", "k31_L10_h1_b.db")]
    packed = str(tmp_path / "packed.db")
    r = subprocess.run([native.KWAGE_DBTOOL_BIN, "repack", packed] + files, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    q = ["-i", os.path.join(cdir, "reads.fastq"), "-i", os.path.join(cdir, "contigs.fa.gz")]
    for K, t in (("2", "0"), ("5", "0.5"), ("1024", "0.8")):
        for fmt in ("csv", "json"):
            a = _run(native.KWAGE_TOP_BIN, ["-d", os.path.join(cdir, "dbs", "a"), "-k", K, "-t", t, "--o." + fmt] + q, cdir)
            b = _run(native.KWAGE_TOP_BIN, ["-d", packed, "-k", K, "-t", t, "--o." + fmt] + q, cdir)
            assert a == b, (K, t, fmt)


def test_file_database_search_sequences_top_agrees_with_kwage_top(native):
    import kwage_amd as ka
    from kwage_amd.engine import FileDatabase
    args, seqs = CASES["basic"]
    cdir = os.path.join(GOLDEN, "basic")
    reads = [l.strip() for l in open(os.path.join(cdir, "q.fa")) if l.strip() and not l.startswith(">")][:6] + seqs
    for K, t in ((3, 0.0), (10, 0.8)):
        rows = _rows(_run(native.KWAGE_TOP_BIN, ["-d", "db", "-k", str(K), "-t", str(t), "--o.csv"] + reads, cdir), "csv")
        with ka.Context(0) as ctx:
            db = FileDatabase(ctx, [os.path.join(cdir, "db")])
            try:
                hits = db.search_sequences_top(reads, K, t)
            finally:
                db.close()
        mine = {}
        for h in hits:
            mine.setdefault("command line seq %d" % h.query, []).append((h.num_kmers_found, h.num_query_kmer, h.accession))
        assert sorted(mine) == sorted(rows)
        for qname, v in rows.items():
            assert [r[:2] for r in v] == [r[:2] for r in mine[qname]], qname
            assert sorted(v) == sorted(mine[qname]), qname
