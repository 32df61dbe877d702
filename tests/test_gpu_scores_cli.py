"""kwage_scores on the reference-written fixtures of tests/golden (basic, multi, k32): the tab-separated matrix equals
FileDatabase.score_matrix on the same queries cell for cell, the header's accessions are score_matrix's, the rows come
in kwage's query order (command-line sequences first, then the records of the -i files), and every score that
`kwage -t 0.5` reports is the cell of its (query, sample)."""
import csv
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = {
    "basic": (["db"], ["q.fa"],
              ["CGGTGTATGTCTTAGTAAATTGTTCAGGACAACTTGTACCCTACTAGGAGGCAGCCGTGTTTGTAAGGCTATTTTGACGTACCGTACTAACATAGCGGCT", "ACGTNACGT"]),
    "multi": (["dbs"], ["reads.fastq", "contigs.fa.gz"], []),
    "k32": (["k32.db"], ["q.fna"], []),
}


@pytest.fixture(scope="module")
def native():
    from kwage_amd import native
    native.ensure_built()
    return native


def read_queries(native, path):
    """[(defline, sequence)] of a FASTA / FASTQ file, as the programs read it (kwage_seqfile_*)."""
    lib = native.lib()
    f = C.c_void_p()
    native.check(lib.kwage_seqfile_open(path.encode(), C.byref(f)))
    out = []
    try:
        while True:
            d, s, n = C.c_char_p(), C.c_char_p(), C.c_uint64()
            r = lib.kwage_seqfile_next(f, C.byref(d), C.byref(s), C.byref(n))
            assert r >= 0
            if r == 0:
                return out
            out.append((d.value.decode("latin-1"), s.value[:n.value].decode("latin-1")))
    finally:
        lib.kwage_seqfile_close(f)


def run_scores(native, args, cwd):
    r = subprocess.run([native.KWAGE_SCORES_BIN] + args, cwd=cwd, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode("latin-1").split("\n")
    assert lines[-1] == ""
    table = [ln.split("\t") for ln in lines[:-1]]
    assert table[0][:2] == ["query", "num_kmers"] and all(len(row) == len(table[0]) for row in table)
    names = [row[0] for row in table[1:]]
    nk = np.array([int(row[1]) for row in table[1:]], dtype=np.uint32)
    cells = np.array([[int(x) for x in row[2:]] for row in table[1:]], dtype=np.uint32).reshape(len(names), len(table[0]) - 2)
    return table[0][2:], names, nk, cells


@pytest.mark.parametrize("case", sorted(CASES))
def test_kwage_scores_equals_score_matrix(native, case, tmp_path):
    import kwage_amd as ka
    from kwage_amd.engine import FileDatabase
    dbs, qfiles, seqs = CASES[case]
    cdir = os.path.join(GOLDEN, case)
    from_files = [rec for f in qfiles for rec in read_queries(native, os.path.join(cdir, f))]
    args = [x for d in dbs for x in ("-d", d)] + [x for f in qfiles for x in ("-i", f)] + seqs
    accessions, names, nk, cells = run_scores(native, args, cdir)
    assert names == ["command line seq %d" % i for i in range(len(seqs))] + [d for d, _ in from_files]
    with ka.Context(0) as ctx:
        db = FileDatabase(ctx, [os.path.join(cdir, d) for d in dbs])
        try:
            matrix, acc = db.score_matrix(seqs + [s for _, s in from_files])
        finally:
            db.close()
    assert matrix.dtype == np.uint32 and matrix.shape == cells.shape and matrix.shape[1] == len(acc) > 0
    assert accessions == acc
    assert np.array_equal(cells, matrix)
    assert cells.any()
    if case != "multi":                                # (one k-mer length: no score above the query's k-mer count)
        assert (cells.max(axis=1) <= nk).all()
    # -o writes the same bytes to a file
    out = str(tmp_path / "m.tsv")
    r = subprocess.run([native.KWAGE_SCORES_BIN] + args + ["-o", out], cwd=cdir, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b""
    again = subprocess.run([native.KWAGE_SCORES_BIN] + args, cwd=cdir, capture_output=True, timeout=120)
    assert open(out, "rb").read() == again.stdout
    # what `kwage -t 0.5` reports for a (query, sample) is that cell (single-parameter databases: one k-mer count per query)
    if case != "multi":
        rep = subprocess.run([native.KWAGE_BIN] + args + ["-t", "0.5", "--o.csv"], cwd=cdir, capture_output=True, timeout=120)
        assert rep.returncode == 0, rep.stderr.decode()
        rows = list(csv.reader(io.StringIO(rep.stdout.decode("latin-1"))))[1:]
        assert rows
        col = {a: i for i, a in enumerate(accessions)}
        assert len(col) == len(accessions)
        for qname, n, found, _, sample in rows:
            q = names.index(qname)
            assert int(n) == nk[q] and int(found) == cells[q, col[sample]], (qname, sample)
