"""A live group model-checked on the device: the operation sequences of tests/group_model.py (a seeded random walk over
file-like blocks, live inserts in their three forms, retires, set_bits, compactions, finalize at a random point, planned
refusals) replayed through the Python objects and the C ABI, and compared with the host model after EVERY operation:
what the call returns (or the error code, with kwage_last_error set), the span, the column count, the row bytes,
real_columns() and every row through read_rows -- all exact.  At the sequence's checkpoints every search form, column_bits
and the filter search are compared with the CPU oracle on the model's matrix and with a cold twin built from that matrix
(group_model.check_all_forms); on the two widest shapes the t = 0.8 early-exit search is repeated with the truncated count
walk and with the screen form forced.  At the end the real columns go through save_db + load and through export_filters +
insert, and must come out as the model's matrix compacted.  tests/test_group_model.py checks the model and the sequences
themselves without a device.

Three orders the sequences were written for, and what they showed on an MI355X:
  1. column_bits(), set_bits on a real column of a finalized group, column_bits() again: Group.set_bits kept the cached
     counts -- confirmed.  Before the fix all nine finalizing default seeds failed at the checkpoint behind their "order1"
     set_bits, seed 0 (shape (0, 300, 5, 1)) first: step 34, column_bits() returned the counts from before the set_bits of
     step 33 (check_all_forms' column_bits comparison).  Fixed: Group.set_bits drops the cache.
  2. a compaction with nothing to close leaves bits planted in the pad columns above the open tail: confirmed, as the model
     says it must -- nothing is launched (seed 0: the compaction of step 38 behind the set_bits of step 37; every seed
     has one).  The header now says so (kwage_group_set_bits, kwage_group_compact), DESIGN.md section 17 too.
  3. set_bits on a finalized group does not re-sample the densities: the truncated count walk, planned with a density_max
     that is wrong about the rows a long query reads (seeds 4, 5, 10: the densest real column filled in exactly those
     rows, the searches at once behind it), reports the oracle's hit lists all the same.  Nothing to fix.
Nothing else surfaced.  Mutations made locally, never committed: without the cache reset in Group.retire_columns the
column_bits comparison of the checkpoint behind a retire fails, and with commit_insert skipping the d_valid upload the
t = 1 hit list of the next checkpoint lacks the inserted columns -- each in all nine finalizing seeds; FileDatabase.compact
keeping its set of retired file columns fails test_file_database_sequences at seeds 1 and 3.

Wall time on one MI355X, the whole -m gpu suite with each file in its own process: 953 s with this file, 934 s for the
files the parent commit has (the same run; a process start, torch's import included, is about 11 s of every file's time);
this file 19 s in its own process (17 s inside pytest, 11 s of them the first test's imports): no sequence takes more
than 1.1 s, a FileDatabase sequence 0.1 s.  tests/test_group_model.py takes 21 s on a CPU.

KWAGE_MODEL_SEEDS in the environment raises the number of seeds (default 12, spread over the six shapes) for a soak."""
import os
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN

import compact_cases as cc
import group_model as gm
import search_shapes as ss

pytestmark = pytest.mark.gpu

CASES = gm.default_cases(max(int(os.environ.get("KWAGE_MODEL_SEEDS", "12")), 1))
STAT_KEYS = ("span_before", "span_after", "columns", "runs", "first_unit", "units")
KERNELS = []                      # (case, knobs' name, search_kernel) of the forced t = 0.8 searches


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


def do_insert(ka, ctx, oracle, g, op, seq, tmp_path, step):
    """The op's filters through the form it names; -> first column."""
    L, _, k, nh = seq.shape
    f = op.filters
    n, fb = f.shape
    if op.form == "host":
        wide = np.full((n, fb + 3), 0xA5, dtype=np.uint8)           # filters 3 bytes further apart than they are long
        wide[:, :fb] = f
        return g.insert_filters(wide)
    if op.form == "device":
        import torch
        wide = np.full((n, (fb + 3) // 4 * 4 + 4), 0x5A, dtype=np.uint8)
        wide[:, :fb] = f
        return g.insert_filters(torch.from_numpy(wide).to(torch.device("cuda", ctx.device)))
    paths = []
    for i in range(n):
        p = str(tmp_path / ("step%d_%d.bloom" % (step, i)))
        oracle.write_bloom(p, k, L, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (1000 * step + i + 1))), f[i])
        paths.append(p)
    return g.insert_bloom_files(paths)


def call(ka, ctx, oracle, g, op, seq, tmp_path, step):
    """The op on the device group -> what the model's method returns for it (the error code where the call is refused)."""
    from kwage_amd.native import lib
    try:
        if op.kind == "add_columns":
            return g.add_columns(op.image, op.nf)
        if op.kind == "insert":
            return do_insert(ka, ctx, oracle, g, op, seq, tmp_path, step)
        if op.kind == "retire":
            g.retire_columns(op.cols)
        elif op.kind == "set_bits":
            g.set_bits(op.rows, op.cols)
        elif op.kind == "compact":
            new, st = g.compact()
            return new, {key: int(st[key]) for key in STAT_KEYS}
        elif op.kind == "finalize":
            g.finalize()
        return 0
    except ka.KwageError as e:
        assert e.code < 0 and lib().kwage_last_error(), (step, op)
        return e.code


def cold_twin(ka, ctx, seq, m):
    """A cold group given the model's matrix as ONE host block, its dead columns withdrawn."""
    L, cap, k, nh = seq.shape
    twin = ka.Group(ctx, k, nh, L, cap)
    assert twin.add_columns(m.packed(), m.span) == 0
    dead = np.flatnonzero(~m.real)
    if dead.size:
        twin.retire_columns(dead)
    twin.finalize()
    return twin


def checkpoint(ka, ctx, oracle, g, m, op, seq, case):
    L, _, k, nh = seq.shape
    twin = cold_twin(ka, ctx, seq, m)
    try:
        gm.check_all_forms(ka, oracle, g, m, ctx, k, nh, L, seq.queries, op.fs, twin=twin)
    finally:
        twin.close()
    if seq.shape in gm.WIDE_SHAPES:
        want = gm.oracle_hits(oracle, m, k, nh, L, seq.queries, 0.8)
        b = ka.Batch(ctx, seq.queries)
        try:
            for name, knobs in (("trunc", ss.TRUNC), ("screen", ss.SCREEN)):
                with ctx.tuning(**knobs):
                    r = g.search(b, 0.8, ka.SEARCH_EARLY_EXIT)
                KERNELS.append((case, name, r.search_kernel, sorted(op.tags)))
                assert [tuple(h) for h in r.hits.tolist()] == want, (case, name, r.search_kernel, sorted(op.tags))
        finally:
            b.close()
    assert not any(ctx.scratch_nonzero().values())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-L%d" % (c[0], c[1][0]))
def test_sequence(ka, ctx, oracle, tmp_path, case):
    seq = gm.sequence(*case)
    L, cap, k, nh = seq.shape
    nrows = 1 << L
    m = gm.GroupModel(L, seq.stride)
    g = ka.Group(ctx, k, nh, L, cap)
    others = []
    try:
        assert g.row_stride == seq.stride
        for step, op in enumerate(seq.ops):
            what = (case, step, op)
            want = m.apply(op)
            if op.kind == "checkpoint":
                if op.search and m.span:
                    try:
                        checkpoint(ka, ctx, oracle, g, m, op, seq, case)
                    except AssertionError as e:
                        raise AssertionError("checkpoint at step %d of seed %d, shape %s" % (step, case[0], case[1])) from e
                continue
            got = call(ka, ctx, oracle, g, op, seq, tmp_path, step)
            if op.kind == "compact":
                assert np.array_equal(got[0], want[0]) and got[1] == {key: want[1][key] for key in STAT_KEYS}, what
            else:
                assert got == want and op.refused() == (got < 0), (what, got, want)
            # the state, all of it, exact (a refused call: the model did not move, so neither may the group)
            assert (g.column_span, g.num_columns, g.row_bytes) == (m.span, m.num_columns, m.span // 8), what
            assert np.array_equal(g.real_columns(), m.real), what
            if m.span:
                rows = g.read_rows(np.arange(nrows))
                assert np.array_equal(rows, m.packed()), (what, np.argwhere(rows != m.packed())[:5])
        # the end: the real columns through a file and back, and through export and insert
        real = np.flatnonzero(m.real)
        assert real.size
        dense = cc.reference(m.bits, m.real)
        path = str(tmp_path / "saved.db")
        g.save_db(path, real.tolist(), [{"run_accession": "SRR%d" % (j + 1)} for j in range(real.size)])
        loaded = ka.Group(ctx, k, nh, L, cap)
        others.append(loaded)
        assert loaded.add_db_file(path) == (0, real.size)
        assert np.array_equal(loaded.read_rows(np.arange(nrows)), dense), case
        filters = g.export_filters(real)
        assert np.array_equal(filters, gm.filters_of(m.bits[:, real])), case
        third = ka.Group(ctx, k, nh, L, cap)
        others.append(third)
        assert third.insert_filters(filters) == 0
        assert np.array_equal(third.read_rows(np.arange(nrows)), dense), case
    finally:
        g.close()
        for o in others:
            o.close()


def test_a_truncated_walk_ran():
    """Across the default seeds the forced searches of the wide shapes' checkpoints reach the truncated count walk (its
    plan reads density_max) and the screen form; needs the sequences above to have run in this process."""
    assert KERNELS, "run together with test_sequence: it collects the kernel names"
    names = [name for _, _, name, _ in KERNELS]
    assert any("trunc>" in n for n in names), Counter(names)
    assert any(n.startswith("count_screen_kernel") for n in names), Counter(names)
    # order 3: a truncated walk planned right behind the set_bits that made a column denser than the last probe saw
    assert any("trunc>" in n and "after_order3" in tags for _, _, n, tags in KERNELS), [(c[0], n, t) for c, _, n, t in KERNELS]


# ----------------------------------------------------------------------------------------------------------------------
# FileDatabase: the second copy of the layout it keeps in Python (_layout, _retired, _LiveBlock), against a model that
# knows only which sample holds which column
# ----------------------------------------------------------------------------------------------------------------------

class DatabaseModel:
    """Run accession -> bool column, per parameter set, in the order a FileDatabase reports samples: the files' samples in
    file order, then the live samples group by group.  Built from the files with the oracle's reader."""

    def __init__(self, oracle, files):
        self.oracle = oracle
        self.files_samples, self.live = [], {}            # [(key, accession, column)]; key -> [(accession, column)]
        for f in files:
            d = oracle.read_db(f)
            h = d.header
            cols = np.unpackbits(np.ascontiguousarray(d.rows), axis=1, bitorder="little")[:, :h.num_filter].astype(bool)
            for j in range(h.num_filter):
                self.files_samples.append(((h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func), d.info(j).csv_string(), cols[:, j].copy()))

    def keys(self):
        return sorted({s[0] for s in self.files_samples} | {key for key, lst in self.live.items() if lst})

    def report(self):
        return self.files_samples + [(key, a, c) for key in self.keys() for a, c in self.live.get(key, [])]

    def group(self, key):
        """The samples of one group in column order."""
        return [s for s in self.files_samples if s[0] == key] + [(key, a, c) for a, c in self.live.get(key, [])]

    def add(self, key, accession, seq):
        k, nh, L, _ = key
        bits = self.oracle.bloom_bits_from_sequences([seq], k, nh, L)
        self.live.setdefault(key, []).append((accession, gm.columns_of(bits[None, :], L)[:, 0]))

    def retire(self, accession):
        for i, s in enumerate(self.files_samples):
            if s[1] == accession:
                del self.files_samples[i]
                return
        for lst in self.live.values():
            for i, s in enumerate(lst):
                if s[0] == accession:
                    del lst[i]
                    return
        raise KeyError(accession)

    def contents(self):
        return Counter((key, a, c.tobytes()) for key, a, c in self.report())

    def counts(self, queries):
        """(int64 [n queries, n samples] in report order, {key: per query distinct k-mers})."""
        report = self.report()
        out = np.zeros((len(queries), len(report)), dtype=np.int64)
        nks = {}
        for key in self.keys():
            k, nh, L, _ = key
            idx = [i for i, s in enumerate(report) if s[0] == key]
            packed = np.ascontiguousarray(np.packbits(np.stack([report[i][2] for i in idx], axis=1), axis=1, bitorder="little"))
            nks[key] = []
            for q, seq in enumerate(queries):
                kmers = self.oracle.unique_kmers(seq, k)
                nks[key].append(len(kmers))
                if len(kmers):
                    for c, m in self.oracle.search_image(packed, packed.shape[1], k, nh, L, len(idx), kmers, 1e-12)[0]:
                        out[q, idx[c]] = m
        return out, nks

    def hits(self, queries, t):
        """Counter of (query, accession, found, distinct k-mers): the oracle's own threshold search, group by group."""
        out = Counter()
        for key in self.keys():
            k, nh, L, _ = key
            mine = self.group(key)
            packed = np.ascontiguousarray(np.packbits(np.stack([s[2] for s in mine], axis=1), axis=1, bitorder="little"))
            for q, seq in enumerate(queries):
                kmers = self.oracle.unique_kmers(seq, k)
                if len(kmers):
                    for c, m in self.oracle.search_image(packed, packed.shape[1], k, nh, L, len(mine), kmers, float(np.float32(t)))[0]:
                        out[(q, mine[c][1], m, len(kmers))] += 1
        return out


def check_database(db, model, queries):
    """search_sequences at 1.0 and 0.8 and score_matrix against the oracle on the model; accessions in report order."""
    report = model.report()
    for t in (1.0, 0.8):
        got = db.search_sequences(queries, t)
        assert Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in got) == model.hits(queries, t), t
        assert [(h.query, -h.num_kmers_found) for h in got] == sorted((h.query, -h.num_kmers_found) for h in got)
    scores, acc = db.score_matrix(queries)
    assert acc == [s[1] for s in report]
    counts, _ = model.counts(queries)
    assert np.array_equal(scores, counts.astype(np.uint32))
    assert sum(g.num_columns for g in db.groups) == len(report)


@pytest.mark.parametrize("seed", range(4))
def test_file_database_sequences(ka, ctx, oracle, tmp_path, seed):
    rng = np.random.default_rng(7000 + seed)
    dbs = os.path.join(GOLDEN, "multi", "dbs")
    fresh = [gm.random_dna(rng, 400) for _ in range(5)]
    reads = [s for _, s in oracle.read_sequences(os.path.join(GOLDEN, "multi", "reads.fastq"))]
    reads = [reads[int(i)] for i in rng.choice(len(reads), size=3, replace=False)]
    queries = reads + [fresh[0][30:200], fresh[1][100:300], fresh[0][:60] + fresh[1][:60], fresh[2][5:150], fresh[3][250:330], "ACGT"]
    plan = ["add", "add", "add", "add", "retire_file", "retire_live", "compact", "compact", "save_reopen", "export"]
    rng.shuffle(plan)
    db = ka.FileDatabase(ctx, [dbs], headroom=64)
    try:
        model = DatabaseModel(oracle, db.files)
        check_database(db, model, queries)
        n_added = 0
        for step, what in enumerate(plan):
            keys = model.keys()
            assert [(g.params.kmer_len, g.params.num_hash, g.params.log_2_filter_len, g.params.hash_func) for g in db.groups] == keys
            live = [a for key in keys for a, _ in model.live.get(key, [])]
            if what == "add":
                gi = int(rng.integers(len(keys)))
                acc = "SRR99%d%02d" % (seed, n_added)
                assert db.add_sample(acc, [fresh[n_added % len(fresh)]], group=gi)[0] == gi
                model.add(keys[gi], acc, fresh[n_added % len(fresh)])
                n_added += 1
            elif what == "retire_live" and live:
                acc = live[int(rng.integers(len(live)))]
                db.retire_sample(acc)
                model.retire(acc)
                with pytest.raises(KeyError):
                    db.retire_sample(acc)
            elif what in ("retire_file", "retire_live"):
                acc = model.files_samples[int(rng.integers(len(model.files_samples)))][1]
                db.retire_sample(acc)
                model.retire(acc)
            elif what == "compact":
                stats = db.compact()
                assert [s["columns"] for s in stats] == [len(model.group(key)) for key in keys]
                assert [g.column_span for g in db.groups] == [(len(model.group(key)) + 7) // 8 * 8 for key in keys]
            elif what == "save_reopen":
                out = str(tmp_path / ("saved%d" % step))
                assert db.save(out)
                db.close()
                db = ka.FileDatabase(ctx, [out], headroom=64)
                again = DatabaseModel(oracle, db.files)            # every sample is a file's now, in the new files' order
                assert again.contents() == model.contents(), (seed, step)
                model = again
            else:
                assert what == "export"
                report = model.report()
                picks = [report[int(i)] for i in rng.choice(len(report), size=3, replace=False)] + [(key, a, c) for key in keys for a, c in model.live.get(key, [])[:1]]
                written = db.export_samples([a for _, a, _ in picks], str(tmp_path / ("bloom%d" % step)))
                assert len(written) == len(picks)
                for key, a, col in picks:
                    params, _, info, bits = oracle.read_bloom(os.path.join(str(tmp_path / ("bloom%d" % step)), a + ".bloom"))
                    assert params == (key[0], key[2], key[1], key[3]) and info.csv_string() == a
                    assert np.array_equal(gm.columns_of(np.ascontiguousarray(bits)[None, :], key[2])[:, 0], col), (seed, step, a)
            check_database(db, model, queries)
        # at the end: the other forms, and the saved directory answers the same
        report = model.report()
        counts, nks = model.counts(queries)
        present, acc = db.presence_matrix(queries, 0.8)
        floors = np.array([[oracle.query_threshold(float(np.float32(0.8)), nks[s[0]][q]) for s in report] for q in range(len(queries))], dtype=np.int64)
        has = np.array([[nks[s[0]][q] > 0 for s in report] for q in range(len(queries))])
        assert acc == [s[1] for s in report] and np.array_equal(present, has & (counts >= floors))
        top = [(h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in db.search_sequences_top(queries, 3)]
        want = []
        for q in range(len(queries)):
            elig = [i for i, s in enumerate(report) if nks[s[0]][q] > 0]
            for i in sorted(elig, key=lambda i: (-counts[q, i], i))[:3]:
                want.append((q, report[i][1], int(counts[q, i]), nks[report[i][0]][q]))
        assert top == want
        asked = [report[0][1], report[-1][1]]
        near = db.similar_samples(asked, 3)
        for (a, recs), want_a in zip(near, asked):
            key = [s[0] for s in report if s[1] == a][0]
            mine = model.group(key)
            A = [s[2] for s in mine if s[1] == a][0]
            cand = []
            for j, (_, a2, col) in enumerate(mine):
                shared, fb, cb = int((A & col).sum()), int(A.sum()), int(col.sum())
                union = fb + cb - shared
                cand.append((-(shared / union if union > 0 else 0.0), j, a2, shared, fb, cb))
            cand.sort()
            assert a == want_a and [(r[0], r[3], r[4], r[5], r[6]) for r in recs] == [(a2, sh, fb, cb, -nj) for nj, _, a2, sh, fb, cb in cand[:3]], (seed, a)
        final = {t: model.hits(queries, t) for t in (1.0, 0.8)}
        out = str(tmp_path / "final")
        assert db.save(out)
    finally:
        db.close()
    again = ka.FileDatabase(ctx, [out])
    try:
        for t in (1.0, 0.8):
            got = Counter((h.query, h.accession, h.num_kmers_found, h.num_query_kmer) for h in again.search_sequences(queries, t))
            assert got == final[t], (seed, t)
    finally:
        again.close()
