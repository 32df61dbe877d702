"""kwage_presence on the reference-written fixtures of tests/golden (basic, multi, k32): the (query, run accession) pairs
whose cell is 1 in `kwage_presence -t T` are exactly the rows `kwage -t T --o.csv` prints, for T = 0.8 and T = 1; the
`passing` column is each row's sum; the rows come in kwage's query order (command-line sequences first, then the records
of the -i files), every query has one; and FileDatabase.presence_matrix gives the same matrix and accessions."""
import csv
import io
import os
import subprocess

import numpy as np
import pytest

from test_gpu_scores_cli import CASES, GOLDEN, read_queries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from kwage_amd import native
    native.ensure_built()
    return native


def run_presence(native, args, cwd):
    r = subprocess.run([native.KWAGE_PRESENCE_BIN] + args, cwd=cwd, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode("latin-1").split("\n")
    assert lines[-1] == ""
    table = [ln.split("\t") for ln in lines[:-1]]
    assert table[0][:3] == ["query", "num_kmers", "passing"] and all(len(row) == len(table[0]) for row in table)
    names = [row[0] for row in table[1:]]
    nk = np.array([int(row[1]) for row in table[1:]], dtype=np.uint32)
    passing = np.array([int(row[2]) for row in table[1:]], dtype=np.uint32)
    assert all(x in ("0", "1") for row in table[1:] for x in row[3:])
    cells = np.array([[x == "1" for x in row[3:]] for row in table[1:]], dtype=bool).reshape(len(names), len(table[0]) - 3)
    return table[0][3:], names, nk, passing, cells, r.stdout


@pytest.mark.parametrize("threshold", ["0.8", "1"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kwage_presence_cells_are_kwages_rows(native, case, threshold, tmp_path):
    import kwage_amd as ka
    from kwage_amd.engine import FileDatabase
    dbs, qfiles, seqs = CASES[case]
    cdir = os.path.join(GOLDEN, case)
    from_files = [rec for f in qfiles for rec in read_queries(native, os.path.join(cdir, f))]
    args = [x for d in dbs for x in ("-d", d)] + [x for f in qfiles for x in ("-i", f)] + seqs
    accessions, names, nk, passing, cells, stdout = run_presence(native, args + ["-t", threshold], cdir)
    assert names == ["command line seq %d" % i for i in range(len(seqs))] + [d for d, _ in from_files]
    assert np.array_equal(passing, cells.sum(axis=1))
    assert len(accessions) > 0
    # the rows `kwage -t T --o.csv` prints
    rep = subprocess.run([native.KWAGE_BIN] + args + ["-t", threshold, "--o.csv"], cwd=cdir, capture_output=True, timeout=120)
    assert rep.returncode == 0, rep.stderr.decode()
    rows = list(csv.reader(io.StringIO(rep.stdout.decode("latin-1"))))[1:]
    theirs = {(qname, sample) for qname, _, _, _, sample in rows}
    mine = {(names[q], accessions[c]) for q, c in np.argwhere(cells).tolist()}
    assert mine == theirs, (sorted(mine - theirs)[:5], sorted(theirs - mine)[:5])
    # the Python counterpart
    with ka.Context(0) as ctx:
        db = FileDatabase(ctx, [os.path.join(cdir, d) for d in dbs])
        try:
            matrix, acc = db.presence_matrix(seqs + [s for _, s in from_files], float(threshold))
        finally:
            db.close()
    assert matrix.dtype == bool and acc == accessions and np.array_equal(matrix, cells)
    # -o writes the same bytes to a file
    out = str(tmp_path / "m.tsv")
    r = subprocess.run([native.KWAGE_PRESENCE_BIN] + args + ["-t", threshold, "-o", out], cwd=cdir, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == stdout
