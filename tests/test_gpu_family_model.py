"""A family of live groups model-checked on the device: the walks of tests/family_model.py (group_model's mutators on
several named groups, Group.fold, Group.copy_columns_from between a fold and a native group of its parameters, groups
created and closed on the way, planned refusals) replayed through the Python objects and compared with the host models
after EVERY step and for EVERY group alive, not only the one the step names: what the call returned (or the error code,
with kwage_last_error set; a refused fold made no group), a fold's stats, the span, the column count, the row bytes, the
row stride, real_columns(), room, and every row through read_rows -- all exact.  At checkpoints on finalized groups every
search form, column_bits and the filter search are compared with the CPU oracle on the model's matrix -- a folded group is
searched with queries hashed at ITS length -- and with a cold twin built from that matrix (group_model.check_all_forms);
on the wide seeds the checkpoint right behind the fold of a finalized group repeats the t = 0.8 early-exit search with the
truncated count walk and with the screen form forced.  At the end every group alive sends its real columns through
save_db + load and through export_filters + insert.  tests/test_family_model.py checks the models and the walks without a
device.

What each order of family_model showed on an MI355X (the 12 default seeds, every one passing on the first run):
  fold_open_tail        as the model says: at tail % 32 = 1, 7, 8 and 31 the insert into the fold and the one into the source
                        land on the same column, each group keeping its own bits below it.
  fold_dirty_above      as the model says: the source shows the bits planted before its compaction as its span grows over
                        them, the fold the OR of them in [row_bytes, 16 U) and zeros from 16 U on.  (A retire clears its
                        columns, so "the memory kept" by a compaction with m == 0 is what set_bits planted in retired
                        columns -- the walk plants them; on finalized groups, which grow by inserts only, no dirty bit
                        ever comes below the span: an insert owns what it grows over.)
  fold_planted          as the model says: planted pad bits and the bits of a retired column are folded and stay masked;
                        a compaction of the fold with nothing to close keeps them, one with something to close clears them.
  fold_empty            as the model says: nothing is launched, the fold of a group that a compaction emptied is all zero
                        where its source is not, inserts and blocks start at column 0.
  fold_final, fold_open as the model says; every search form right behind the fold of a finalized group equals the oracle
                        (the fold's own density probe), add_columns is refused with ERR_STATE, inserts are taken.
  fold_twice            L -> L1 -> L2 and L -> L2 give the same device group.
  fold_then_close_src   as the model says: the fold is mutated and searched to the end of the walk with its source gone;
                        in the other half of the seeds the source lives on and stays what its model says.
  copy_from_fold, copy_into_fold, the refusals
                        as the model says.
  the forced searches   seeds 0 and 6 (wide, R finalized before the fold): count_walk_kernel<..,trunc> and
                        count_screen_kernel ran on the freshly folded group and reported the oracle's hit lists.
Nothing to fix: no bug surfaced in fold.hip, copy.hip, insert.hip, compact.hip or engine.py, and the header already says
what the model says.  Mutations made locally, never committed, and the part that catches each:
  - Group.fold not copying _tail (the fold's mirror says "tail closed"): test_sequence fails at the first fold of an open
    tail -- seed 0, step 7, `room` 8832 against the model's 8927;
  - fold.hip not taking over tail_open: test_sequence fails at the insert into the fold behind it -- seed 0, step 8, first
    column 384 (the next 16-byte boundary) against the model's 289;
  - merge_groups not re-indexing _retired: test_file_database_sequences (tests/test_gpu_group_model.py) fails at all four
    seeds in the check behind the merge -- the sample retired in the last group, whose index the merge moves, is reported again.

Wall time on one MI355X: this file 17 s inside pytest in a process of its own (13 s of them the first test: imports and
the first use of the device); no sequence takes more than 1.1 s, a wide one 0.6 to 1.1 s, a narrow one 0.1 to 0.25 s.  In
the whole -m gpu suite run in ONE process (814 s, 1199 tests) this file is 4.3 s, so the files the parent commit has are
810 s of the same run; tests/test_gpu_group_model.py is 6.3 s of it, a FileDatabase sequence with the new steps 0.09 s.
tests/test_family_model.py takes 13 s on a CPU (the not-gpu suite: 375 s with it).

KWAGE_MODEL_SEEDS in the environment raises the number of seeds (default 12) for a soak."""
import os
import types
from collections import Counter

import numpy as np
import pytest

import compact_cases as cc
import family_model as fm
import group_model as gm
import search_shapes as ss
from test_gpu_group_model import STAT_KEYS, cold_twin, do_insert

pytestmark = pytest.mark.gpu

SEEDS = fm.default_seeds(max(int(os.environ.get("KWAGE_MODEL_SEEDS", "12")), 1))
FOLD_KEYS = ("log_2_before", "log_2_after", "units_per_row", "bytes_read", "bytes_written")
KERNELS = []                      # (seed, knobs' name, search_kernel, the checkpoint's tags) of the forced t = 0.8 searches


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


def as_one(seq, L):
    """What group_model's helpers read of a sequence, for a group of 2^L rows of this family."""
    _, cap, k, nh = seq.shape
    return types.SimpleNamespace(shape=(L, cap, k, nh))


def call(ka, ctx, oracle, groups, models, op, seq, tmp_path, step, stats=None):
    """The step on the device groups -> what the family returns for it (the error code where the call is refused); a
    union's stats go into `stats`."""
    from kwage_amd.native import lib
    _, cap, k, nh = seq.shape
    try:
        if op.kind == "new":
            groups[op.on] = ka.Group(ctx, k, nh, op.L, cap)
            return 0
        if op.kind == "close":
            groups.pop(op.on).close()
            return 0
        if op.kind == "fold":
            made, st = groups[op.src].fold(op.L2)
            groups[op.on] = made
            return {key: int(st[key]) for key in FOLD_KEYS}
        g = groups[op.on]
        if op.kind == "copy":
            return g.copy_columns_from(groups[op.src], op.cols)[0]
        if op.kind == "union":
            first, st = g.union_columns(op.sets, groups[op.src])
            if stats is not None:
                stats.update(st)
            return first
        if op.kind == "add_columns":
            return g.add_columns(op.image, op.nf)
        if op.kind == "insert":
            return do_insert(ka, ctx, oracle, g, op, as_one(seq, g.params.log_2_filter_len), tmp_path, step)
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


def checkpoint(ka, ctx, oracle, g, m, op, seq):
    _, _, k, nh = seq.shape
    one = as_one(seq, m.L)
    twin = cold_twin(ka, ctx, one, m)
    try:
        gm.check_all_forms(ka, oracle, g, m, ctx, k, nh, m.L, seq.queries, op.fs, twin=twin)
    finally:
        twin.close()
    if seq.wide and "after_fold_final" in op.tags:
        want = gm.oracle_hits(oracle, m, k, nh, m.L, seq.queries, 0.8)
        b = ka.Batch(ctx, seq.queries)
        try:
            for name, knobs in (("trunc", ss.TRUNC), ("screen", ss.SCREEN)):
                with ctx.tuning(**knobs):
                    r = g.search(b, 0.8, ka.SEARCH_EARLY_EXIT)
                KERNELS.append((seq.seed, name, r.search_kernel, sorted(op.tags)))
                assert [tuple(h) for h in r.hits.tolist()] == want, (seq.seed, name, r.search_kernel, sorted(op.tags))
        finally:
            b.close()
    assert not any(ctx.scratch_nonzero().values())


def check_every_group(groups, fam, op, packed, what):
    """The state of EVERY group alive behind a step, all of it, exact; packed: name -> the model's rows packed, until a step
    names the group."""
    assert sorted(groups) == sorted(fam.models), what          # (a refused fold made no group)
    for name in (op.on, getattr(op, "src", None)):
        packed.pop(name, None)
    for name, m in fam.models.items():
        g = groups[name]
        assert (g.column_span, g.num_columns, g.row_bytes, g.row_stride) == (m.span, m.num_columns, m.span // 8, m.stride), (what, name)
        assert g.params.log_2_filter_len == m.L and np.array_equal(g.real_columns(), m.real), (what, name)
        assert g.room == max(0, m.room()), (what, name, g.room, m.room())
        if m.span:
            if name not in packed:
                packed[name] = m.packed()
            rows = g.read_rows(np.arange(m.nrows))
            assert np.array_equal(rows, packed[name]), (what, name, np.argwhere(rows != packed[name])[:5])
    if hasattr(op, "twin"):               # fold_twice, union_fold_commutes: the two device groups are the same
        a, b = groups[op.on], groups[op.twin]
        nrows = np.arange(fam.models[op.on].nrows)
        assert (a.column_span, a.num_columns) == (b.column_span, b.num_columns) and np.array_equal(a.real_columns(), b.real_columns())
        assert np.array_equal(a.read_rows(nrows), b.read_rows(nrows)), what


def round_trips(ka, ctx, groups, fam, seq, tmp_path, others):
    """The end: every group's real columns through a file and back, and through export and insert."""
    _, cap, k, nh = seq.shape
    seed = seq.seed
    for name, m in fam.models.items():
        g, real = groups[name], np.flatnonzero(m.real)
        if not real.size:
            continue
        nrows = np.arange(m.nrows)
        dense = cc.reference(m.bits, m.real)
        path = str(tmp_path / ("saved_%s.db" % name))
        g.save_db(path, real.tolist(), [{"run_accession": "SRR%d" % (j + 1)} for j in range(real.size)])
        loaded = ka.Group(ctx, k, nh, m.L, cap)
        others.append(loaded)
        assert loaded.add_db_file(path) == (0, real.size)
        assert np.array_equal(loaded.read_rows(nrows), dense), (seed, name)
        filters = g.export_filters(real)
        assert np.array_equal(filters, gm.filters_of(m.bits[:, real])), (seed, name)
        third = ka.Group(ctx, k, nh, m.L, cap)
        others.append(third)
        assert third.insert_filters(filters) == 0
        assert np.array_equal(third.read_rows(nrows), dense), (seed, name)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(ka, ctx, oracle, tmp_path, seed):
    seq = fm.sequence(seed)
    fam, groups, others = fm.Family(seq.shape), {}, []
    packed = {}                                   # name -> the model's rows packed, until a step names the group
    try:
        for step, op in enumerate(seq.ops):
            what = (seed, step, op)
            want = fam.apply(op)
            if op.kind == "checkpoint":
                if op.search:
                    try:
                        checkpoint(ka, ctx, oracle, groups[op.on], fam.models[op.on], op, seq)
                    except AssertionError as e:
                        raise AssertionError("checkpoint at step %d of seed %d on %s" % (step, seed, op.on)) from e
                continue
            got = call(ka, ctx, oracle, groups, fam.models, op, seq, tmp_path, step)
            if op.kind == "compact":
                assert np.array_equal(got[0], want[0]) and got[1] == {key: want[1][key] for key in STAT_KEYS}, what
            else:
                assert got == want and op.refused() == (isinstance(got, int) and got < 0), (what, got, want)
            check_every_group(groups, fam, op, packed, what)
        round_trips(ka, ctx, groups, fam, seq, tmp_path, others)
    finally:
        for g in list(groups.values()) + others:
            g.close()


def test_a_truncated_walk_ran_on_a_fresh_fold():
    """Across the default seeds the forced searches right behind the fold of a finalized wide group reach the truncated
    count walk (its plan reads the density_max the fold sampled itself) and the screen form; needs the sequences above to
    have run in this process."""
    assert KERNELS, "run together with test_sequence: it collects the kernel names"
    assert all("after_fold_final" in tags for _, _, _, tags in KERNELS)
    names = [name for _, _, name, _ in KERNELS]
    assert any("trunc>" in n for n in names), Counter(names)
    assert any(n.startswith("count_screen_kernel") for n in names), Counter(names)
