"""The union of columns model-checked on the device in walks: the sequences of tests/union_walk.py (group_model's mutators
on several named groups, Group.fold, Group.union_columns within one group and between two, groups created and closed on
the way, planned refusals) replayed through the Python objects and compared with the host models after EVERY step and for
EVERY group alive: what the call returned (or the error code, with kwage_last_error set), a union's stats (sets, members,
entries, first_unit, units, bytes_written), the span, the column count, the row bytes, the row stride, real_columns(), room,
and every row through read_rows -- all exact.  At checkpoints on finalized groups every search form, column_bits (0 on
every skipped or retired column) and the filter search are compared with the CPU oracle on the model's matrix and with a
cold twin built from it (group_model.check_all_forms), and the context's scratch is all zero.  At the end every group alive
sends its real columns through save_db + load and through export_filters + insert.  The step, the checkpoint and the
per-step comparison are tests/test_gpu_family_model.py's.  tests/test_union_walk.py checks the walks without a device.

What each order of union_walk showed on an MI355X (the 12 default seeds, every one passing on the first run):
  union_same_open_tail  as the model says: at tail % 128 = 1, 31, 33 and 127 the union lands at the next multiple of 128,
                        the insert continues right behind it and a block lands at the 16-byte boundary behind that.
  union_over_dirty      as the model says: the columns a same-group union skips keep the bits the memory held (planted by
                        set_bits in retired columns before a compaction with m == 0) and come below the span as dead
                        columns: real_columns(), every search form, column_bits (0 there), the later compaction, save_db
                        and export_filters leave them out (seeds 4 and 10, finalized: searched right behind the union);
                        the bytes above the union's last 32-bit word in its own unit keep what they held and show it once
                        a block brings them below the span (seeds 1 and 7, open).
  union_of_unions       as the model says: a union whose members an earlier launch stored is the flat union of the originals.
  union_merge           as the model says; the compaction behind the retire of all members closes the union's pad gap too.
  union_into_fold, union_from_fold, union_within_fold, union_fold_commutes
                        as the model says, folds at L = 5, 3 and 0 included; union then fold and fold then the same union
                        give the same device group, the folded pad gap included.
  union_final, union_open, union_above_kib, union_full_row, the refusals
                        as the model says: every search form right behind a union into a finalized group equals the oracle
                        (on the wide seeds with union columns on both sides of column 8192), a union that ends on the
                        row's last column leaves room 0 and one more set is refused, every refusal leaves every group as
                        it was.
Nothing to fix: no bug surfaced in union.hip, union_plan.hpp, union_kernels.hpp, insert.hip, compact.hip, fold.hip or
engine.py.  The header now says what the model says about the columns a same-group union skips.  Mutations made locally,
never committed, and the part that catches each:
  - Group.union_columns not calling _inserted: test_sequence fails at every seed's first union -- seed 0, step 6, group R:
    real_columns() does not show the new column (the comparison in front of `room`'s, which the same mirror feeds);
  - plan_union passing dst_tail_open without `&& !same_group`: test_sequence fails at every seed's union_same_open_tail --
    seed 0, step 6: first column 385 against the model's 512; seed 1, step 5: 287 against 384; seed 2, step 6: 289 against
    384 -- and tests/test_union_walk.py::test_every_union_equals_the_planners fails at every seed's first union step (seed
    0: units [3, 4) are written where [4, 5) are expected);
  - union_columns_kernel with keeps_high forced false: seeds 1 and 7 (union_over_dirty on an open group) fail at the reveal
    block that brings the bytes below the span -- seed 1, step 36 and seed 7, step 34, group D: read_rows differs from the
    model in bytes 20 .. 31 of a row (seed 1: rows 3, 6, 8, 9, 11 ... at bytes 22, 23, 29, 28, 31), where the bits planted
    before the compaction are gone; the other ten seeds pass;
  - FileDatabase.union_samples(retire=True) not updating _retired, and _renumbered recording f0 for f0 + c:
    test_file_database_sequences (tests/test_gpu_group_model.py) fails at all four seeds, see there.

Wall time on one MI355X: in the whole -m gpu suite run in ONE process (832 s, 1306 tests) this file is 6.8 s, so the files
the parent commit has are 825 s of the same run; a wide sequence takes 1.1 to 1.5 s (its widest group, 8264 columns of
2^11 rows, is searched in every form and closed), a narrow one 0.15 to 0.27 s; a FileDatabase sequence with the union
steps 0.11 s (0.09 s before).  In a process of its own this file takes 20 s, 13 s of them the first test's imports and
first use of the device.  tests/test_union_walk.py takes 26 s on a CPU (the not-gpu suite: 423 s with it, 586 tests).

KWAGE_MODEL_SEEDS in the environment raises the number of seeds (default 12) for a soak."""
import os

import numpy as np
import pytest

import family_model as fm
import union_walk as uw
from test_gpu_family_model import call, check_every_group, checkpoint, round_trips
from test_gpu_group_model import STAT_KEYS

pytestmark = pytest.mark.gpu

SEEDS = uw.default_seeds(max(int(os.environ.get("KWAGE_MODEL_SEEDS", "12")), 1))
UNION_KEYS = ("first_column", "sets", "members", "entries", "first_unit", "units", "bytes_written")


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


def implied_stats(op, first, nrows):
    """What the model implies for the stats of a union that landed at `first`."""
    n = len(op.sets)
    units = (first + n + 127) // 128 - first // 128
    return {"first_column": first, "sets": n, "members": sum(len(s) for s in op.sets), "entries": sum(len({c // 32 for c in s}) for s in op.sets),
            "first_unit": first // 128, "units": units, "bytes_written": nrows * units * 16}


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(ka, ctx, oracle, tmp_path, seed):
    seq = uw.sequence(seed)
    fam, groups, others = fm.Family(seq.shape), {}, []
    packed = {}
    try:
        for step, op in enumerate(seq.ops):
            what = (seed, step, op)
            want = fam.apply(op)
            if op.kind == "checkpoint":
                if op.search:
                    try:
                        checkpoint(ka, ctx, oracle, groups[op.on], fam.models[op.on], op, seq)
                    except AssertionError as e:
                        raise AssertionError("checkpoint at step %d of seed %d on %s (%s)" % (step, seed, op.on, sorted(op.tags))) from e
                continue
            stats = {}
            got = call(ka, ctx, oracle, groups, fam.models, op, seq, tmp_path, step, stats)
            if op.kind == "compact":
                assert np.array_equal(got[0], want[0]) and got[1] == {key: want[1][key] for key in STAT_KEYS}, what
            else:
                assert got == want and op.refused() == (isinstance(got, int) and got < 0), (what, got, want)
            if op.kind == "union" and not op.refused():
                assert {key: int(stats[key]) for key in UNION_KEYS} == implied_stats(op, want, fam.models[op.on].nrows), (what, stats)
            check_every_group(groups, fam, op, packed, what)
        round_trips(ka, ctx, groups, fam, seq, tmp_path, others)
    finally:
        for g in list(groups.values()) + others:
            g.close()
