"""kwage_near on the reference-written fixtures of tests/golden/multi: the whole output for two run accessions that lie
in different files equals a numpy computation from the files' own slices (kwage_db_read_slices): shared, query and sample
bit counts as popcounts, the Jaccard index in float64, each query's lines under (Jaccard descending, file order, column
ascending).  Files with other Bloom parameters are skipped with a line on stderr."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = os.path.join(ROOT, "tests", "golden", "multi")
FILES = ["dbs/a/k31_L10_h1.db", "dbs/k31_L12_h3.db", "dbs/a/deeper/k31_L10_h1_b.db", "dbs/b/k15_L11_h2.DB"]       # database order: as given


@pytest.fixture(scope="module")
def native():
    from kwage_amd import native
    native.ensure_built()
    return native


def load(native, path):
    """(header, run accessions, bool [2^L, num_filter] columns) of one .db file, from the file alone."""
    lib = native.lib()
    h = native.DbHeader()
    native.check(lib.kwage_db_read_header(path.encode(), C.byref(h)))
    d = C.c_void_p()
    native.check(lib.kwage_dbinfo_open(path.encode(), C.byref(d)))
    buf = C.create_string_buffer(64)
    names = []
    for c in range(h.num_filter):
        native.check(lib.kwage_dbinfo_csv_string(d, c, buf, 64))
        names.append(buf.value.decode())
    lib.kwage_dbinfo_close(d)
    rows = np.arange(1 << h.log_2_filter_len, dtype=np.uint32)
    out = np.zeros((rows.size, (h.num_filter + 7) // 8), dtype=np.uint8)
    native.check(lib.kwage_db_read_slices(path.encode(), rows.ctypes.data_as(C.POINTER(C.c_uint32)), rows.size, out.ctypes.data_as(C.c_void_p)))
    return h, names, np.unpackbits(out, axis=1, bitorder="little")[:, :h.num_filter].astype(bool)


def expected_lines(dbs, queries, k):
    lines = ["query\trank\tsample\tshared_bits\tquery_bits\tsample_bits\tjaccard"]
    for acc in queries:
        fq, cq = next((fi, names.index(acc)) for fi, (_, names, _) in enumerate(dbs) if acc in names)
        hq, _, bq = dbs[fq]
        f = bq[:, cq]
        cand = []
        for fi, (h, names, bits) in enumerate(dbs):
            if (h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func) != (hq.kmer_len, hq.num_hash, hq.log_2_filter_len, hq.hash_func):
                continue
            for c in range(h.num_filter):
                shared, sb = int((f & bits[:, c]).sum()), int(bits[:, c].sum())
                union = int(f.sum()) + sb - shared
                jac = np.float64(shared) / np.float64(union) if union else np.float64(0)
                cand.append((-jac, fi, c, names[c], shared, sb))
        cand.sort(key=lambda t: t[:3])
        for r, (nj, _, _, name, shared, sb) in enumerate(cand[:k]):
            lines.append("%s\t%d\t%s\t%d\t%d\t%d\t%.6f" % (acc, r + 1, name, shared, int(f.sum()), sb, -nj))
    return lines


@pytest.mark.parametrize("k", [3, 1024])
def test_kwage_near_equals_numpy(native, tmp_path, k):
    dbs = [load(native, os.path.join(MULTI, f)) for f in FILES]
    # one query sample from the first file, one from the third (the same parameters, a later file), the first one again through -s
    queries = [dbs[2][1][4], dbs[0][1][0], dbs[0][1][12]]
    args = [x for f in FILES for x in ("-d", f)] + ["-k", str(k), "-o", str(tmp_path / "near.tsv"), queries[0], "-s", queries[1], queries[2]]
    r = subprocess.run([native.KWAGE_NEAR_BIN] + args, cwd=MULTI, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "", r
    got = (tmp_path / "near.tsv").read_text().split("\n")
    assert got[-1] == ""
    # (-s accessions come before the positional ones)
    exp = expected_lines(dbs, [queries[1], queries[0], queries[2]], k)
    assert got[:-1] == exp, [(a, b) for a, b in zip(got, exp) if a != b][:5]
    # every query sample finds itself with 1.000000 at the top (no identical filter precedes it in these files)
    firsts = [ln.split("\t") for ln in got[1:-1] if ln.split("\t")[1] == "1"]
    assert [(f[0], f[2], f[6]) for f in firsts] == [(q, q, "1.000000") for q in (queries[1], queries[0], queries[2])]
    skipped = [ln for ln in r.stderr.split("\n") if ln]
    assert len(skipped) == 6 and all(ln.startswith("Skipping dbs/") and "parameters differ" in ln for ln in skipped), r.stderr
