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

test_file_database_sequences also holds FileDatabase.fold, reserve and merge_groups (and a live sample added under a file
sample's accession), shuffled in with the older steps on a directory built for it: three files that share (k, num_hash,
hash_func) at L = 12, 10, 10 and one at other parameters BEHIND them, so that a merge moves its group's index.  Its
DatabaseModel is a list of groups in db.groups order, every sample knowing where it came from; the report order is restated
from the doc-strings of _blocks and merge_groups.  On an MI355X all four seeds answer as the model says; merge_groups not
re-indexing _retired (a local mutation) fails all four in the check behind the merge.

It holds FileDatabase.union_samples as well (database_plan: union, union_dup, union_last_group, union_across -- refused
between the fold and the merge, taken behind it --, union_of_union, retire_union_member, retire_udup): DatabaseModel.unions
resolves every member by "first in report order" before anything changes and places the new samples, live ones, behind
the group's others.  (Which file's samples come first in report order follows the directory listing, so the members a
seed picks differ from one file system to the next; the steps choose among what is there.)  On an MI355X all four seeds
answer as the model says after every step.  Two mutations, made locally: union_samples(retire=True) not updating _retired
fails all four seeds in the union_last_group step (retire_sample of a member that is gone finds it again and
kwage_group_retire_columns refuses "column 1 is a pad column", or _retired has no entry of the last group);
_renumbered recording f0 for f0 + c fails all four in check_database behind the first step that cuts a block -- a
compact or the merge -- where the search reports a sample under its block's first accession.

Wall time on one MI355X, the whole -m gpu suite with each file in its own process: 953 s with this file, 934 s for the
files the parent commit has (the same run; a process start, torch's import included, is about 11 s of every file's time);
this file 19 s in its own process (17 s inside pytest, 11 s of them the first test's imports): no sequence takes more
than 1.1 s, a FileDatabase sequence 0.1 s.  tests/test_group_model.py takes 21 s on a CPU.

KWAGE_MODEL_SEEDS in the environment raises the number of seeds (default 12, spread over the six shapes) for a soak."""
import os
from collections import Counter

import numpy as np
import pytest

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
    """The groups of a FileDatabase in db.groups order: each its parameters and its samples in COLUMN order, a sample
    being (where it came from, run accession, bool column) -- it came from (0, file index, column in the file) or, added
    live, from (1, serial number).  Built from the files with the oracle's reader, as FileDatabase groups them: by
    parameters, sorted, a group's files in file order.

    The report order is restated from the doc-strings of FileDatabase._blocks and merge_groups: the files' samples in
    file order (a file's in column order), then the live samples group by group in column order; a merged group stands at
    the place of its first member and holds its members' samples in member order."""

    def __init__(self, oracle, files):
        self.oracle, self.n_live = oracle, 0
        by = {}
        for fi, f in enumerate(files):
            d = oracle.read_db(f)
            h = d.header
            cols = np.unpackbits(np.ascontiguousarray(d.rows), axis=1, bitorder="little")[:, :h.num_filter].astype(bool)
            for j in range(h.num_filter):
                by.setdefault((h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func), []).append(((0, fi, j), d.info(j).csv_string(), cols[:, j].copy()))
        self.groups = [[key, samples] for key, samples in sorted(by.items())]        # [parameters, [(origin, accession, column)]]

    def keys(self):
        return [key for key, _ in self.groups]

    def report(self):
        """[(parameters, accession, column, group index, origin)] in report order."""
        everything = [(key, a, c, gi, origin) for gi, (key, samples) in enumerate(self.groups) for origin, a, c in samples]
        return sorted((s for s in everything if s[4][0] == 0), key=lambda s: s[4]) + [s for s in everything if s[4][0] == 1]

    def group(self, gi):
        """The samples of one group in column order, as report() lists them."""
        key, samples = self.groups[gi]
        return [(key, a, c, gi, origin) for origin, a, c in samples]

    def live(self):
        return [s[1] for s in self.report() if s[4][0] == 1]

    def add(self, gi, accession, seq):
        """A live sample: its filter built at the length the group has NOW, its column behind every other of the group."""
        k, nh, L, _ = self.groups[gi][0]
        bits = self.oracle.bloom_bits_from_sequences([seq], k, nh, L)
        self.groups[gi][1].append(((1, self.n_live), accession, gm.columns_of(bits[None, :], L)[:, 0]))
        self.n_live += 1

    def first(self, accession):
        """The first sample in report order carrying the accession; KeyError where none does."""
        for s in self.report():
            if s[1] == accession:
                return s
        raise KeyError(accession)

    def unions(self, unions, retire=False):
        """FileDatabase.union_samples: [(new accession, member accessions)] -> [group index] of the new samples.  Every
        member is resolved by "first in report order" BEFORE anything changes (KeyError for an unknown one, ValueError for
        members in two groups); each new sample is a live one, its column the OR of its members', placed behind the
        group's others in the order of the list; with retire the resolved members go afterwards."""
        resolved = [[self.first(a) for a in members] for _, members in unions]
        for members in resolved:
            if len({s[3] for s in members}) != 1:
                raise ValueError("members in two groups")
        for (new, _), members in zip(unions, resolved):
            gi = members[0][3]
            self.groups[gi][1].append(((1, self.n_live), new, np.any([s[2] for s in members], axis=0)))
            self.n_live += 1
        if retire:
            for gi, origin in {(s[3], s[4]) for members in resolved for s in members}:
                self.groups[gi][1][:] = [s for s in self.groups[gi][1] if s[0] != origin]
        return [members[0][3] for members in resolved]

    def union(self, new_accession, member_accessions, retire=False):
        return self.unions([(new_accession, list(member_accessions))], retire)[0]

    def retire(self, accession):
        """The first sample in report order carrying the accession is withdrawn -> (group index, where it came from)."""
        for key, a, c, gi, origin in self.report():
            if a == accession:
                self.groups[gi][1][:] = [s for s in self.groups[gi][1] if s[0] != origin]
                return gi, origin
        raise KeyError(accession)

    def fold(self, L2):
        """Every group with longer filters: its columns folded by GroupModel's rule, row r' the OR of rows r' + j * 2^L2.
        -> the group indices folded."""
        done = []
        for gi, (key, samples) in enumerate(self.groups):
            k, nh, L, hf = key
            if L > L2:
                self.groups[gi] = [(k, nh, L2, hf), [(origin, a, c.reshape(1 << (L - L2), 1 << L2).any(axis=0)) for origin, a, c in samples]]
                done.append(gi)
        return done

    def merge(self):
        """Groups that share their parameters become one at the place of the first -> [member indices] of every group of
        the new list."""
        members = {}
        for gi, (key, _) in enumerate(self.groups):
            members.setdefault(key, []).append(gi)
        groups, made = [], []
        for gi, (key, _) in enumerate(self.groups):
            if members[key][0] == gi:
                groups.append([key, [s for g2 in members[key] for s in self.groups[g2][1]]])
                made.append(members[key])
        self.groups = groups
        return made

    def contents(self):
        return Counter((key, a, c.tobytes()) for key, a, c, _, _ in self.report())

    def counts(self, queries):
        """(int64 [n queries, n samples] in report order, {parameters: per query distinct k-mers})."""
        report = self.report()
        out = np.zeros((len(queries), len(report)), dtype=np.int64)
        nks = {}
        for gi, (key, samples) in enumerate(self.groups):
            k, nh, L, _ = key
            nks[key] = [len(self.oracle.unique_kmers(seq, k)) for seq in queries]
            idx = [i for i, s in enumerate(report) if s[3] == gi]
            if not idx:
                continue
            packed = np.ascontiguousarray(np.packbits(np.stack([report[i][2] for i in idx], axis=1), axis=1, bitorder="little"))
            for q, seq in enumerate(queries):
                kmers = self.oracle.unique_kmers(seq, k)
                if len(kmers):
                    for c, m in self.oracle.search_image(packed, packed.shape[1], k, nh, L, len(idx), kmers, 1e-12)[0]:
                        out[q, idx[c]] = m
        return out, nks

    def hits(self, queries, t):
        """Counter of (query, accession, found, distinct k-mers): the oracle's own threshold search, group by group."""
        out = Counter()
        for gi, (key, samples) in enumerate(self.groups):
            k, nh, L, _ = key
            if not samples:
                continue
            packed = np.ascontiguousarray(np.packbits(np.stack([s[2] for s in samples], axis=1), axis=1, bitorder="little"))
            for q, seq in enumerate(queries):
                kmers = self.oracle.unique_kmers(seq, k)
                if len(kmers):
                    for c, m in self.oracle.search_image(packed, packed.shape[1], k, nh, L, len(samples), kmers, float(np.float32(t)))[0]:
                        out[(q, samples[c][1], m, len(kmers))] += 1
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
    assert [g.num_columns for g in db.groups] == [len(samples) for _, samples in model.groups]


DB_FILES = [("a.db", (21, 2, 12), range(0, 5)), ("b.db", (21, 2, 10), range(5, 9)), ("c.db", (21, 2, 10), range(9, 12)),
            ("d.db", (25, 2, 11), range(12, 16))]          # (d.db: the group BEHIND those a fold makes equal -- a merge moves its index)


def build_directory(ctx, oracle, tmp_path, seqs):
    """`.db` files under tmp_path/src from oracle-built `.bloom` files: three that share (k, num_hash, hash_func) at
    L = 12, 10, 10 and one at other parameters; sample i is SRR<8300 + i>."""
    import ctypes as C
    from kwage_amd.native import lib, check, Params
    src = tmp_path / "src"
    src.mkdir()
    for name, (k, nh, lg), members in DB_FILES:
        paths = []
        for i in members:
            p = str(tmp_path / ("SRR%d_L%d.bloom" % (8300 + i, lg)))
            oracle.write_bloom(p, k, lg, nh, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (8300 + i))),
                               oracle.bloom_bits_from_sequences([seqs[i]], k, nh, lg))
            paths.append(p)
        prm = Params(k, nh, lg, 0)
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        check(lib().kwage_build_db(ctx._h, str(src / name).encode(), C.byref(prm), arr, len(paths), None))
    return str(src)


def database_plan(rng, seed):
    """The steps of a seed: the old kinds and fold, merge, reserve, add_dup shuffled together, under the order every seed
    keeps -- a retire_file before the fold, the fold before the merge (a retire in the LAST group between them, nothing
    compacted: the merge has a retired file column to re-index), and a retire, a compact and a save_reopen behind the merge.
    Seed 1 reserves between the fold and the merge, the others behind the merge.  FileDatabase.union_samples goes with
    them: before the fold `union` (two unions in one call: a live block of two samples; two file samples and a live one
    are members) and `union_dup` (the new sample takes a FILE sample's accession); between the fold and the merge
    `union_last_group` (retire=True in the last group: _retired entries and a live block of two for the merge to re-index)
    and `union_across` (members in the two groups that share parameters since the fold: ValueError); behind the merge the
    same `union_across` list (it succeeds), `union_of_union` (a member that is an earlier union sample),
    `retire_union_member` (the middle sample of a live block of three, before the part's compact, which cuts the block)
    and `retire_udup` (the accession of union_dup resolves to the file's sample)."""
    first = ["add", "add", "retire_file", "compact", "add_dup", "export", "union", "union_dup"]
    between = ["add", "retire_dup", "retire_last_group", "union_last_group", "union_across"] + (["reserve"] if seed == 1 else [])
    after = ["retire_live", "retire_file", "compact", "save_reopen", "add", "retire_dup2", "export", "union_across", "union_of_union", "retire_union_member",
             "retire_udup"] + ([] if seed == 1 else ["reserve"])
    for part in (first, between, after):
        rng.shuffle(part)
    a, b = after.index("retire_union_member"), after.index("compact")      # (the compaction cuts the block the retire left a hole in)
    if a > b:
        after[a], after[b] = after[b], after[a]
    a, b = between.index("retire_last_group"), between.index("union_last_group")      # (the union's retire leaves the last group's files to the retire before it)
    if a > b:
        between[a], between[b] = between[b], between[a]
    return first + ["fold"] + between + ["merge"] + after


@pytest.mark.parametrize("seed", range(4))
def test_file_database_sequences(ka, ctx, oracle, tmp_path, seed):
    rng = np.random.default_rng(7000 + seed)
    seqs = [gm.random_dna(rng, 300) for _ in range(16)]
    dbs = build_directory(ctx, oracle, tmp_path, seqs)
    fresh = [gm.random_dna(rng, 400) for _ in range(5)]
    picks = [int(i) for i in rng.choice(16, size=3, replace=False)]
    queries = [seqs[picks[0]][10:150], seqs[picks[1]][50:250], seqs[picks[2]], fresh[0][30:200], fresh[1][100:300], fresh[0][:60] + fresh[1][:60],
               fresh[2][5:150], fresh[3][250:330], seqs[2][:60] + seqs[7][:60], "ACGT"]
    plan = database_plan(rng, seed)
    assert plan.index("retire_file") < plan.index("fold") < plan.index("merge") < min(len(plan) - 1 - plan[::-1].index(w) for w in ("retire_file", "compact", "save_reopen"))
    assert (plan.index("fold") < plan.index("reserve") < plan.index("merge")) == (seed == 1)
    params_of = lambda g: (g.params.kmer_len, g.params.num_hash, g.params.log_2_filter_len, g.params.hash_func)
    db = ka.FileDatabase(ctx, [dbs], headroom=64)
    try:
        model = DatabaseModel(oracle, db.files)
        assert [key[2] for key in model.keys()] == [10, 12, 11] and [len(s) for _, s in model.groups] == [7, 5, 4]
        check_database(db, model, queries)
        n_added, dup, udup, n_unions = 0, None, None, 0
        across, unioned = None, []                  # the members of union_across; the accessions the union steps made, oldest first
        protected = set()                        # accessions a later step names: the random retires leave them alone

        def fresh_union():
            nonlocal n_unions
            n_unions += 1
            return "SRR77%d%02d" % (seed, n_unions)

        def union_call(unions, retire=False):
            """One union_samples call against the model: the new samples' groups, their columns consecutive per group."""
            want = model.unions(unions, retire)
            got = db.union_samples(unions, retire=retire)
            assert [gi for gi, _ in got] == want, (got, want)
            for gi in set(want):
                cols = [c for g2, c in got if g2 == gi]
                assert cols == list(range(cols[0], cols[0] + len(cols))) and cols[0] % 128 == 0
            unioned.extend(new for new, _ in unions)

        def others_of(gi, n=None, file_only=False):
            """The accessions of group gi's samples that resolve to themselves (dup and udup left out), file samples first:
            n of them, or all.  (Which file's samples come first in report order is the directory listing's choice.)"""
            mine = [s for s in model.report() if s[3] == gi and model.first(s[1])[4] == s[4] and (s[4][0] == 0 or not file_only) and s[1] not in (dup, udup)]
            assert n is None or len(mine) >= n, (gi, n, len(mine))
            return [s[1] for s in mine[:n]]

        for step, what in enumerate(plan):
            keys = model.keys()
            assert [params_of(g) for g in db.groups] == keys
            live = [a for a in model.live() if a not in protected]
            if what == "add":
                gi = int(rng.integers(len(keys)))
                acc = "SRR99%d%02d" % (seed, n_added)
                assert db.add_sample(acc, [fresh[n_added % len(fresh)]], group=gi)[0] == gi
                model.add(gi, acc, fresh[n_added % len(fresh)])          # (behind a fold: hashed at the group's new length)
                n_added += 1
            elif what == "add_dup":
                # a live sample under a FILE sample's accession: the file's comes first in report order
                dup = [s for s in model.report() if s[4][0] == 0][int(rng.integers(3))][1]
                gi = int(rng.integers(len(keys)))
                assert db.add_sample(dup, [fresh[4]], group=gi)[0] == gi
                model.add(gi, dup, fresh[4])
            elif what in ("retire_dup", "retire_dup2"):
                carriers = [s for s in model.report() if s[1] == dup]
                assert len(carriers) == (2 if what == "retire_dup" else 1)
                gi, origin = model.retire(dup)
                assert origin == carriers[0][4] and db.retire_sample(dup)[0] == gi
                if what == "retire_dup":
                    assert origin[0] == 0 and [s[4][0] for s in model.report() if s[1] == dup] == [1]      # the file's went, the live one stays
                else:
                    with pytest.raises(KeyError):
                        db.retire_sample(dup)
            elif what == "retire_live" and [a for a in live if a != dup]:
                acc = [a for a in live if a != dup][int(rng.integers(len([a for a in live if a != dup])))]
                assert db.retire_sample(acc)[0] == model.retire(acc)[0]
                with pytest.raises(KeyError):
                    db.retire_sample(acc)
            elif what in ("retire_file", "retire_live", "retire_last_group"):
                mine = [s for s in model.report() if s[4][0] == 0 and s[1] != dup and s[1] not in protected and (what != "retire_last_group" or s[3] == len(keys) - 1)]
                acc = mine[int(rng.integers(len(mine)))][1]
                assert db.retire_sample(acc)[0] == model.retire(acc)[0]
            elif what == "union":
                # two file samples and one live sample of one group, two unions in ONE call: a live block of two samples
                with_live = sorted({s[3] for s in model.report() if s[4][0] == 1 and model.first(s[1])[4] == s[4]})
                if not with_live:
                    gi = int(rng.integers(len(keys)))
                    acc = "SRR99%d%02d" % (seed, n_added)
                    assert db.add_sample(acc, [fresh[n_added % len(fresh)]], group=gi)[0] == gi
                    model.add(gi, acc, fresh[n_added % len(fresh)])
                    n_added += 1
                    with_live = [gi]
                gi = with_live[int(rng.integers(len(with_live)))]
                f1, f2 = others_of(gi, 2, file_only=True)
                lv = [s[1] for s in model.report() if s[3] == gi and s[4][0] == 1 and model.first(s[1])[4] == s[4]][0]
                state = [(g.column_span, g.num_columns) for g in db.groups]
                with pytest.raises(KeyError):
                    db.union_samples([(fresh_union(), [f1, "SRR7777777"])])
                with pytest.raises(KeyError):
                    model.union("SRR0", [f1, "SRR7777777"])
                assert [(g.column_span, g.num_columns) for g in db.groups] == state
                union_call([(fresh_union(), [f1, lv, f2]), (fresh_union(), [f2, f2])])
                protected.add(unioned[-2])                          # (union_of_union names it)
            elif what == "union_dup":
                # the new sample takes a FILE sample's accession: retire_sample and a later union resolve to the file's
                files = [s for s in model.report() if s[4][0] == 0 and s[1] != dup and s[1] not in protected and s[3] != len(keys) - 1]
                carrier = files[int(rng.integers(len(files)))]
                udup = carrier[1]
                protected.add(udup)
                union_call([(udup, others_of(carrier[3], 2))])
                unioned.pop()
                assert [s[4][0] for s in model.report() if s[1] == udup] == [0, 1] and model.first(udup)[4] == carrier[4]
            elif what == "retire_udup":
                carriers = [s for s in model.report() if s[1] == udup]
                gi, origin = model.retire(udup)
                assert origin == carriers[0][4] and db.retire_sample(udup)[0] == gi
                assert len([s for s in model.report() if s[1] == udup]) == len(carriers) - 1
            elif what == "union_last_group":
                gi = len(keys) - 1
                f1 = others_of(gi, 1, file_only=True)[0]                     # (four file samples, at most three retired by now)
                f2 = ([a for a in others_of(gi) if a != f1] + [f1])[0]
                union_call([(fresh_union(), [f1, f2]), (fresh_union(), [f1])], retire=True)
                assert any(g2 == gi for g2, _ in db._retired) and any(len(e[2].accessions) == 2 for e in db._layout[gi] if hasattr(e[2], "accessions"))
                with pytest.raises(KeyError):
                    db.retire_sample(f1)
            elif what == "union_across":
                if across is None:
                    # members in the two groups that share their parameters since the fold: refused until they are merged
                    assert keys[0] == keys[1]
                    across = [others_of(0, 1, file_only=True)[0], others_of(1, 1, file_only=True)[0]]
                    protected.update(across)
                    state = [(g.column_span, g.num_columns) for g in db.groups]
                    with pytest.raises(ValueError, match=r"fold\(\) and merge_groups\(\) first"):
                        db.union_samples([(fresh_union(), [across[0]]), (fresh_union(), across)])
                    with pytest.raises(ValueError):
                        model.union("SRR0", across)
                    assert [(g.column_span, g.num_columns) for g in db.groups] == state
                else:
                    union_call([(fresh_union(), across)])
                    protected.difference_update(across)
            elif what == "union_of_union":
                # one member is an earlier union sample (a file sample by now where a save_reopen came in between)
                earlier = unioned[0]
                gi = model.first(earlier)[3]
                union_call([(fresh_union(), [earlier] + [a for a in others_of(gi) if a != earlier][:1])])
                protected.discard(earlier)
            elif what == "retire_union_member":
                # the middle sample of a live block of three goes; the part's compact, which follows, cuts the block in two
                roomy = [g2 for g2 in range(len(keys)) if len(others_of(g2)) >= 2]
                gi = roomy[int(rng.integers(len(roomy)))]
                a, b = others_of(gi, 2)
                block = [fresh_union() for _ in range(3)]
                union_call([(block[0], [a]), (block[1], [a, b]), (block[2], [b])])
                assert any(getattr(e[2], "accessions", None) == block for e in db._layout[gi])
                assert db.retire_sample(block[1])[0] == model.retire(block[1])[0] == gi
                assert (gi, [e for e in db._layout[gi] if getattr(e[2], "accessions", None) == block][0][0] + 1) in db._retired
                assert "compact" in plan[step + 1:]
                unioned.remove(block[1])
            elif what == "compact":
                stats = db.compact()
                assert [s["columns"] for s in stats] == [len(samples) for _, samples in model.groups]
                assert [g.column_span for g in db.groups] == [(len(samples) + 7) // 8 * 8 for _, samples in model.groups]
            elif what == "fold":
                old = list(db.groups)
                done = model.fold(10)
                stats = db.fold(10)
                assert [(s["log_2_before"], s["log_2_after"]) for s in stats] == [(keys[gi][2], 10) for gi in done] and len(done) == 2
                assert all((db.groups[gi] is not old[gi]) == (gi in done) and bool(old[gi]._h) == (gi not in done) for gi in range(len(old)))
                assert len(model.keys()) == len(keys) and len(set(model.keys())) == len(keys) - 1      # two groups share their parameters until a merge
                assert db.fold(10) == []
            elif what == "merge":
                old, strides = list(db.groups), [g.row_stride for g in db.groups]
                made = model.merge()
                assert db.merge_groups() == len(old) - len(made) == 1
                assert [params_of(g) for g in db.groups] == model.keys()
                for g, members in zip(db.groups, made):
                    if len(members) > 1:
                        assert 8 * g.row_stride == sum(8 * strides[gi] for gi in members) and not any(old[gi]._h for gi in members)
                    else:
                        assert g is old[members[0]]
                assert db.merge_groups() == 0
            elif what == "reserve":
                old = list(db.groups)
                h = max(g.room for g in old) + 1
                stats = db.reserve(h)
                assert all(g.room >= h for g in db.groups) and not any(g in old for g in db.groups) and not any(g._h for g in old)
                assert len(stats) == len(old) and [s["columns"] for s in stats if s] == [len(samples) for _, samples in model.groups if samples]
                assert db.reserve(h) == []
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
                picks = [report[int(i)] for i in rng.choice(len(report), size=3, replace=False)] + [s for s in report if s[4][0] == 1][:2]
                picks += [s for s in report if s[1] in unioned][-1:]                # (a union sample)
                assert "merge" not in plan[:step] or any(s[1] in unioned for s in picks)
                first = {}
                for s in report:
                    first.setdefault(s[1], s)
                picks = list({s[1]: first[s[1]] for s in picks}.values())      # (an accession carried twice: the first in report order is written, once)
                written = db.export_samples([s[1] for s in picks], str(tmp_path / ("bloom%d" % step)))
                assert len(written) == len(picks)
                for key, a, col, _, _ in picks:
                    params, _, info, bits = oracle.read_bloom(os.path.join(str(tmp_path / ("bloom%d" % step)), a + ".bloom"))
                    assert params == (key[0], key[2], key[1], key[3]) and info.csv_string() == a
                    assert np.array_equal(gm.columns_of(np.ascontiguousarray(bits)[None, :], key[2])[:, 0], col), (seed, step, a)
            try:
                check_database(db, model, queries)
            except AssertionError as e:
                raise AssertionError("after step %d (%s) of seed %d: %s" % (step, what, seed, plan)) from e
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
            mine = [s for gi in range(len(model.groups)) if model.keys()[gi] == key for s in model.group(gi)]      # (group order, then column order)
            A = [s[2] for s in report if s[1] == a][0]
            cand = []
            for j, (_, a2, col, _, _) in enumerate(mine):
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
