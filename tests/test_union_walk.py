"""The walks of tests/union_walk.py checked without a device -- every sequence that tests/test_gpu_union_walk.py replays on
the GPU is inspected here first.

  1. the walks are deterministic, at most 60 steps long, never have more than five groups alive, and no matrix is larger
     than 2^11 rows of 1152 bytes;
  2. a second statement of the union: after every successful `union` step the destination is, up to the stride, what a
     plain loop over sets and members makes of the state before -- dst[r, first + j] = any(src[r, c] for c in set j), zero
     from the new tail to the end of its 32-bit word, everything else as it was -- with `first` computed here: the open tail
     between two groups, the next multiple of 128 at or above the span within one; every model the step does not name, and
     every model after a refused step, is as before;
  3. the library's own planning: tests/sanitize/union_walk_driver.cpp, built with g++ -fsanitize=address,undefined as a
     stand-alone program and run as a child process, takes every union step of the default walks as text (state, lists, the
     source's rows) through union_refusal, plan_union, union_unit_value and copy_keep_mask over every row and unit; the
     refusal or `first`, the stats and every row written equal the model's, exactly;
  4. a ledger over the 12 default seeds: every order, list kind, tail % 128 residue and refusal union_walk names occurs,
     finalized and open destinations each within one group and between two, and each order has the steps around it that
     its description promises;
  5. what keeps the device checkpoints from being vacuous: every finalizing seed ends in a searched checkpoint on a group
     with valid union columns, at every searched checkpoint at least half of the group's valid union columns have fill
     below 0.9, and the oracle reports the union of the two samples for the queries cut from either and for the query made
     of halves of both, which neither member answers.
Nothing of the library is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import family_model as fm
import group_model as gm
import union_model as um
import union_walk as uw

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")
SEEDS = uw.default_seeds(max(int(os.environ.get("KWAGE_MODEL_SEEDS", "12")), 12))
ERROR_WORDS = {"refuse_own_fold": "log_2_filter_len differs", "refuse_retired": "pad or retired", "refuse_pad": "pad or retired", "refuse_beyond": "beyond the span",
               "refuse_empty_set": "is empty", "refuse_no_sets": "n_sets is 0", "refuse_capacity": "capacity exceeded"}


@pytest.fixture(scope="module")
def sequences():
    return {seed: uw.sequence(seed) for seed in SEEDS}


def replay(seq):
    """(step, op, the family before, the family after, {group: its union columns}) for every step of a walk; a column is
    a union column from the union that made it on, through folds and compactions, until it is retired."""
    fam, made = fm.Family(seq.shape), {}
    for step, op in enumerate(seq.ops):
        before = fam.copy()
        r = fam.apply(op)
        assert results_equal(r, op.result), (seq.seed, step, op)
        if not op.refused():
            if op.kind == "new":
                made[op.on] = set()
            elif op.kind == "close":
                del made[op.on]
            elif op.kind == "fold":
                made[op.on] = set(made[op.src])
            elif op.kind == "union":
                made[op.on] |= set(range(r, r + len(op.sets)))
            elif op.kind == "retire":
                made[op.on] -= set(int(c) for c in op.cols)
            elif op.kind == "compact":
                made[op.on] = {int(r[0][c]) for c in made[op.on]}
            for name, m in fam.models.items():
                assert all(m.valid[c] for c in made[name]), (seq.seed, step, name)
        yield step, op, before, fam, made


def results_equal(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and np.array_equal(a[0], b[0]) and a[1] == b[1]
    return a == b


def landing(m, same):
    """Where a union lands, stated once more: the open tail between two groups, the next multiple of 128 at or above the
    span within one."""
    if not same and m.tail_open:
        return m.tail_column
    return (m.span + 127) // 128 * 128


# ----------------------------------------------------------------------------------------------------------------------
# 1. determinism and limits
# ----------------------------------------------------------------------------------------------------------------------

def test_walks_are_deterministic_short_and_small(sequences):
    for seed in SEEDS[:12]:
        a, b = sequences[seed], uw.sequence(seed)
        assert a.queries == b.queries and len(a.ops) == len(b.ops)
        for x, y in zip(a.ops, b.ops):
            assert (x.kind, x.on, x.tags) == (y.kind, y.on, y.tags) and results_equal(x.result, y.result)
            for key in ("image", "filters", "rows", "cols", "fs", "src", "L2", "L", "twin"):
                assert np.array_equal(getattr(x, key, None), getattr(y, key, None)), (seed, x, key)
            assert getattr(x, "sets", None) == getattr(y, "sets", None), (seed, x)      # (lists of unequal lengths)
    for seed, seq in sequences.items():
        assert 25 <= len(seq.ops) <= uw.MAX_STEPS == 60, (seed, len(seq.ops))
        assert seq.shape == (fm.WIDE if seed % 3 == 0 else fm.NARROW)
        for step, op, _, fam, _ in replay(seq):
            assert 1 <= len(fam.models) <= uw.MAX_ALIVE == 5, (seed, op)
            for m in fam.models.values():
                assert m.nrows <= 1 << seq.shape[0] <= 1 << 11 and m.stride == seq.stride <= 1152
        assert seq.ops[-1].kind == "checkpoint" and "last" in seq.ops[-1].tags and 10 <= len(seq.queries) <= 16


# ----------------------------------------------------------------------------------------------------------------------
# 2. a second statement of the union
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_every_union_equals_a_second_statement(sequences, seed):
    seq = sequences[seed]
    unions = 0
    for step, op, before, fam, _ in replay(seq):
        what = (seed, step, op)
        if op.refused():
            assert fam.same(before), what
            continue
        for name, m in fam.models.items():
            if name != op.on and name in before.models:
                assert m.same(before.models[name]), (what, name)
        if op.kind != "union":
            continue
        unions += 1
        same = op.on == op.src
        dst0, src0, dst = before.models[op.on], before.models[op.src], fam.models[op.on]
        n = len(op.sets)
        first = landing(dst0, same)
        assert op.result == first and first + n <= 8 * dst0.stride, (what, first)
        want = dst0.matrix.copy()
        for j, members in enumerate(op.sets):                       # rows at once: one numpy column per member
            column = np.zeros(dst0.nrows, dtype=bool)
            for c in members:
                column = column | src0.matrix[:, c]
            want[:, first + j] = column
        for r in range(0, dst0.nrows, 37 if dst0.nrows > 64 else 1):      # and bit by bit
            for j in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
                assert bool(want[r, first + j]) == any(bool(src0.matrix[r, c]) for c in op.sets[j]), (what, r, j)
        word_end = ((first + n - 1) // 32 + 1) * 32
        want[:, first + n:word_end] = False
        assert want.shape[1] == 8 * dst.stride and np.array_equal(dst.matrix, want), (what, np.argwhere(dst.matrix != want)[:5])
        valid = dst0.valid.copy()
        valid[first:first + n] = True
        assert np.array_equal(dst.valid, valid) and not dst0.valid[first:].any(), what
        assert (dst.tail_open, dst.tail_column, dst.next_byte, dst.finalized, dst.L) == (True, first + n, (first + n + 7) // 8, dst0.finalized, dst0.L), what
        assert all(c < src0.span and src0.valid[c] for s in op.sets for c in s) and src0.L == dst0.L, what
    assert unions >= 10, (seed, unions)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the planners
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("union_walk")
    exe = str(tmp / "union_walk_driver")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "union_walk_driver.cpp"), "-o", exe, "-lz", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]

    def run(text, n_ops):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr or "ReserveShadowMemoryRange failed" in r.stderr):
            pytest.skip("the sanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0][:200])
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
        assert "no report" in r.stdout and not any(x in r.stderr for x in REPORTS), r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert out[-1] == "%d operations, no report" % n_ops
        return out[:-1]

    return run


def hex_rows(packed):
    return [row.tobytes().hex() or "-" for row in packed]


def stream_and_expectation(seq):
    """(the driver's input, the lines the model says it must print, what each line belongs to) for one walk's union steps."""
    text, want, where = [], [], []
    n_ops = 0
    for step, op, before, fam, _ in replay(seq):
        if op.kind != "union":
            continue
        n_ops += 1
        same = op.on == op.src
        dst0, src0 = before.models[op.on], before.models[op.src]
        n, members = len(op.sets), sum(len(s) for s in op.sets)
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in op.sets], dtype=np.int64)]).astype(np.int64)
        first = landing(dst0, same)
        if op.refused():
            nrows, src_bytes, unit0, units = 0, 0, 0, 0
        else:
            nrows, src_bytes = dst0.nrows, min((src0.span + 31) // 32 * 4, src0.stride)
            unit0, units = first // 128, (first + n + 127) // 128 - first // 128
        head = "union %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (same, dst0.L, src0.L, dst0.next_byte, dst0.tail_open, dst0.tail_column, dst0.stride, src0.span,
                                                                    src0.stride, nrows, src_bytes, unit0, units, n, members)
        text.append(head)
        text.append(np.packbits(src0.real, bitorder="little").tobytes().hex() or "-")
        text.append(" ".join(map(str, offsets.tolist())))
        text.append(" ".join(str(c) for s in op.sets for c in s) or " ")
        if op.refused():
            tag = [t for t in op.tags if t.startswith("refuse_")][0]
            want.append(("union rc=%d error=" % op.result, ERROR_WORDS[tag]))
            where.append((seq.seed, step, op))
            continue
        text += hex_rows(np.packbits(src0.matrix, axis=1, bitorder="little")[:, :src_bytes])
        text += hex_rows(np.packbits(dst0.matrix, axis=1, bitorder="little")[:, 16 * unit0:16 * (unit0 + units)])
        entries = sum(len({c // 32 for c in s}) for s in op.sets)
        want.append("union rc=0 first=%d sets=%d members=%d entries=%d first_unit=%d units=%d bytes_written=%d"
                    % (op.result, n, members, entries, op.result // 128, units, dst0.nrows * units * 16))
        where.append((seq.seed, step, op))
        after = np.packbits(fam.models[op.on].matrix, axis=1, bitorder="little")[:, 16 * unit0:16 * (unit0 + units)]
        for r, row in enumerate(hex_rows(after)):
            want.append("w " + row)
            where.append((seq.seed, step, op, "row %d" % r))
    return "".join(x + "\n" for x in text), want, where, n_ops


@pytest.mark.parametrize("seed", SEEDS)
def test_every_union_equals_the_planners(driver, sequences, seed):
    text, want, where, n_ops = stream_and_expectation(sequences[seed])
    got = driver(text, n_ops)
    assert len(got) == len(want), (seed, len(got), len(want))
    for g, w, at in zip(got, want, where):
        if isinstance(w, tuple):
            # (the capacity is the live insert's refusal, plan_insert's, in its own words)
            assert g.startswith(w[0]) and w[1] in g and ("kwage_group_union_columns" in g or w[1] == "capacity exceeded"), (at, g, w)
        else:
            assert g == w, (at, g[:200], w[:200])


# ----------------------------------------------------------------------------------------------------------------------
# 4. the ledger
# ----------------------------------------------------------------------------------------------------------------------

def test_ledger(sequences):
    default = {seed: seq for seed, seq in sequences.items() if seed < 12}
    assert len(default) == 12
    seeds_with, combos, own_fold = {}, set(), set()
    for seed, seq in default.items():
        ops = seq.ops
        steps = {step: (before, {name: m.copy() for name, m in fam.models.items()}) for step, op, before, fam, _ in replay(seq)
                 if op.tags & {"union_over_dirty", "union_full_row", "union_fold_commutes", "union_same_open_tail"}}
        assert seq.finalizes == (seed % 4 != 3)
        for i, op in enumerate(ops):
            assert op.refused() == any(t.startswith("refuse_") for t in op.tags), (seed, op)
            for t in op.tags:
                seeds_with.setdefault(t, set()).add(seed)
            if op.kind != "union":
                continue
            assert op.tags & {"same_group", "two_group"} == {"same_group" if op.on == op.src else "two_group"}
            if "refuse_own_fold" in op.tags:
                own_fold.add("into" if "dst_fold" in op.tags else "from")
            if op.refused():
                continue
            n = len(op.sets)
            combos.add(("dst_final" if "dst_final" in op.tags else "dst_open", "same_group" if op.on == op.src else "two_group"))
            rest = [o for o in ops[i + 1:] if o.on == op.on]
            if "union_same_open_tail" in op.tags:
                before = steps[i][0].models[op.on]
                assert op.on == op.src and before.tail_open and before.tail_column % 128 in uw.RESIDUES and op.result == (before.tail_column + 127) // 128 * 128
                assert rest[0].kind == "insert" and rest[0].result == op.result + n, (seed, rest[0])
                if "dst_open" in op.tags:
                    assert rest[1].kind == "add_columns" and rest[1].result == (op.result + n + len(rest[0].filters) + 127) // 128 * 128
            if "union_final" in op.tags:
                assert "dst_final" in op.tags and ops[i + 1].kind == "checkpoint" and ops[i + 1].on == op.on and ops[i + 1].search and op.result in ops[i + 1].fs
                assert rest[1].kind == "add_columns" and rest[1].result == uw.ERR_STATE
            if "union_open" in op.tags:
                assert "dst_open" in op.tags and ops[i + 1].kind == "add_columns" and ops[i + 1].on == op.on and ops[i + 1].result >= op.result + n
            if "union_over_dirty" in op.tags:
                before, after = steps[i][0].models[op.on], steps[i][1][op.on]
                prev = [o for o in ops[:i] if o.on == op.on]
                assert [o.kind for o in prev[-4:]] == ["retire", "set_bits", "compact", "insert"] and prev[-2].result[1]["columns"] == 0
                word_end = ((prev[-1].result + len(prev[-1].filters) - 1) // 32 + 1) * 32
                assert op.on == op.src and word_end < op.result and after.matrix[:, word_end:op.result].any() and not after.valid[word_end:op.result].any()
                last_word = ((op.result + n - 1) // 32 + 1) * 32
                assert last_word % 128 and after.matrix[:, last_word:(last_word + 127) // 128 * 128].any()
                if "dst_open" in op.tags:
                    assert rest[0].kind == "add_columns" and "reveal" in rest[0].tags and not rest[0].refused() and rest[0].result >= (last_word + 127) // 128 * 128
                else:
                    assert ops[i + 1].kind == "checkpoint" and ops[i + 1].on == op.on and ops[i + 1].search
                tail = [o.kind for o in rest if o.kind in ("compact", "insert", "checkpoint")]
                assert tail[-3:] == ["compact", "insert", "checkpoint"] and [o for o in rest if o.kind == "compact"][0].result[1]["units"] > 0
            if "union_full_row" in op.tags:
                after = steps[i][1][op.on]
                assert after.span == 8 * after.stride and after.room() == 0 and n == 8 * after.stride - landing(steps[i][0].models[op.on], op.on == op.src)
                assert "refuse_capacity" in ops[i + 1].tags and len(ops[i + 1].sets) == 1 and ops[i + 1].on == op.on
            if "union_above_kib" in op.tags:
                assert seq.wide and op.result == 8064 and n >= 200 and op.result + n > 8192
                cp = [o for o in rest if o.kind == "checkpoint"][0]
                assert any(op.result <= c < 8192 for c in cp.fs) and any(8192 <= c < op.result + n for c in cp.fs)
                assert (rest[0].kind == "finalize" and cp.search) or not seq.finalizes
            if "union_merge" in op.tags:
                assert [o.kind for o in rest[:4]] == ["retire", "compact", "insert", "checkpoint"]
                assert sorted(set(rest[0].cols)) == sorted({c for s in op.sets for c in s}) and sorted(g for g in rest[2].genomes if g >= 0) == list(range(6))
            if hasattr(op, "twin"):
                after = steps[i][1]
                assert "union_fold_commutes" in op.tags and after[op.on].same(after[op.twin]) and after[op.on].L == after[op.twin].L
                src = [o for o in ops[:i] if o.kind == "union" and "union_fold_commutes" in o.tags][-1]
                assert src.sets == op.sets and src.result == op.result and src.result > 0
                folds = [o for o in ops[:i] if o.kind == "fold" and "union_fold_commutes" in o.tags][-2:]
                assert [f.on for f in folds] == [op.on, op.twin] and folds[0].src == folds[1].src == src.on and ops.index(folds[0]) < ops.index(src) < ops.index(folds[1])
                gap = steps[ops.index(src)][0].models[src.on]
                assert gap.tail_open and gap.tail_column % 128, "the pad gap is folded too"
    for t in uw.ORDERS + tuple("refuse_" + r for r in uw.REFUSALS) + tuple("list_" + k for k in um.LISTS) + tuple("tail%%128=%d" % r for r in uw.RESIDUES):
        assert seeds_with.get(t), t
        if t != "union_above_kib":
            assert len(seeds_with[t]) >= 2, (t, seeds_with[t])
    assert seeds_with["union_above_kib"] == {s for s in default if s % 3 == 0}
    assert combos == {(a, b) for a in ("dst_final", "dst_open") for b in ("same_group", "two_group")}, combos
    for t in ("union_final", "union_open"):
        for how in ("same_group", "two_group"):
            assert any(t in op.tags and how in op.tags for seq in default.values() for op in seq.ops), (t, how)
    assert own_fold == {"into", "from"}
    for L2 in (5, 3, 0):
        assert any({"union_within_fold", "to%d" % L2} <= op.tags for seq in default.values() for op in seq.ops), L2
    assert any("union_over_dirty" in op.tags and "dst_open" in op.tags for seq in default.values() for op in seq.ops)
    assert any("union_over_dirty" in op.tags and "dst_final" in op.tags for seq in default.values() for op in seq.ops)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the checkpoints are not vacuous
# ----------------------------------------------------------------------------------------------------------------------

def test_checkpoints_are_not_vacuous(sequences, oracle):
    for seed, seq in sequences.items():
        if seed >= 12:
            continue
        _, _, k, nh = seq.shape
        searched = 0
        for step, op, _, fam, made in replay(seq):
            if op.kind != "checkpoint" or not op.search:
                continue
            searched += 1
            m = fam.models[op.on]
            cols = sorted(made[op.on])
            assert cols and m.finalized, (seed, step, op)
            fill = m.matrix[:, cols].sum(axis=0) / m.nrows
            assert 2 * int((fill < 0.9).sum()) >= len(cols) and fill.min() > 0, (seed, step, op, np.round(fill, 2))
        last = seq.ops[-1]
        assert (last.kind, last.search) == ("checkpoint", seq.finalizes) and bool(searched) == seq.finalizes, seed
        if not seq.finalizes:
            continue
        # the union of the samples queries 1 and 2 were cut from, in the group the last checkpoint searches
        union = [o for o in seq.ops if "genome_union" in o.tags][-1]
        assert seq.ops[-2] is union and union.on == last.on
        u, g1, g2 = union.result, union.sets[0][0], union.sets[0][1]
        assert u in made[last.on] and last.fs == sorted([u, g1, g2])
        for g, c in ((1, g1), (2, g2)):
            exact = gm.columns_of(oracle.bloom_bits_from_sequences([seq.genomes[g]], k, nh, m.L)[None, :], m.L)[:, 0]
            assert np.array_equal(m.matrix[:, c], exact), (seed, g)
        assert seq.queries[1] == seq.genomes[1][1:] and seq.queries[2] == seq.genomes[2][:-1]
        h = len(seq.genomes[1]) // 2
        assert seq.queries[-1] == seq.genomes[1][:h] + "N" + seq.genomes[2][:h]
        at1 = {(q, c) for q, c, _ in gm.oracle_hits(oracle, m, k, nh, m.L, seq.queries, 1.0)}
        halves = len(seq.queries) - 1
        assert (1, u) in at1 and (2, u) in at1 and (1, g1) in at1 and (2, g2) in at1, seed
        assert (halves, u) in at1 and (halves, g1) not in at1 and (halves, g2) not in at1, seed
