"""The model of tests/group_model.py and its operation sequences, checked without a device -- every sequence that
tests/test_gpu_group_model.py replays on the GPU is inspected here first.

  1. the model against the library's own planners: tests/sanitize/group_model_driver.cpp, built with
     g++ -fsanitize=address,undefined as a stand-alone program, runs plan_insert / insert_span / plan_retire / plan_compact /
     compact_fill_map / compact_valid_mask on the operation stream of every default (seed, shape); what each call returns
     (refusals included) and the state it leaves -- span, tail, column count, the valid mask, the column map, runs and
     units of a compaction -- must equal the model's, which restates the rules from the header without calling them;
  2. the model against a second statement of the same thing: every column gets an identity when it enters; at every
     checkpoint the real columns in ascending order are the surviving identities in entry order, each holding its entry
     bits OR-ed with what set_bits planted while it was real, and after a compaction the matrix is
     compact_cases.reference of the matrix before it;
  3. a ledger over the default seeds: every operation kind, insert residue, boundary crossing, retire form, refusal and
     each of the three orders the sequences were written for occurs, and the CPU oracle on the model finds at each
     finalizing seed's last checkpoint a hit at t = 1, a pair that passes at 0.8 only, a query with k-mers and no hit, and
     neighbouring real columns with different scores.
Nothing of the library is loaded into python."""
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT

import compact_cases as cc
import group_model as gm

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")
CASES = gm.default_cases()


@pytest.fixture(scope="module")
def sequences():
    return {case: gm.sequence(*case) for case in CASES}


# ----------------------------------------------------------------------------------------------------------------------
# 1. the planners
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("group_model")
    exe = str(tmp / "group_model_driver")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "group_model_driver.cpp"), "-o", exe, "-lz", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]

    def run(lines):
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr or "ReserveShadowMemoryRange failed" in r.stderr):
            pytest.skip("the sanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0][:200])
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
        assert "no report" in r.stdout and not any(x in r.stderr for x in REPORTS), r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines) + 1 and out[-1] == "%d operations, no report" % len(lines)
        return out[:-1]

    return run


def fold(new_column):
    """The column map as the driver prints it: src:dst:len of every stretch of columns whose new numbers count up with them."""
    out, c, n = [], 0, len(new_column)
    while c < n:
        if new_column[c] < 0:
            c += 1
            continue
        ln = 1
        while c + ln < n and new_column[c + ln] == new_column[c] + ln:
            ln += 1
        out.append("%d:%d:%d" % (c, new_column[c], ln))
        c += ln
    return ",".join(out) or "-"


def state_text(m):
    return "span=%d open=%d tail=%d columns=%d valid=%s" % (m.span, m.tail_open, m.tail_column, m.num_columns,
                                                              np.packbits(m.real, bitorder="little").tobytes().hex())


def stream_and_expectation(seq):
    """(the driver's input, the lines the model says it must print) for one sequence."""
    m = gm.GroupModel(seq.shape[0], seq.stride)
    lines, want = ["new %d" % seq.stride], ["new rc=0 | " + state_text(m)]
    for op in seq.ops:
        if op.kind == "checkpoint":
            continue
        r = m.apply(op)
        rc = r if isinstance(r, int) and r < 0 else 0
        if op.kind == "add_columns":
            lines.append("add %d" % op.nf)
            text = "add rc=%d first=%d" % (rc, 0 if rc else r)
        elif op.kind == "insert":
            n = len(op.filters)
            lines.append("ins %d" % n)
            text = "ins rc=%d first=%d word_first=%d word_last=%d keep=%d" % ((rc, 0, 0, 0, 0) if rc else (0, r, r // 32, (r + n - 1) // 32, r % 32))
        elif op.kind == "retire":
            lines.append("ret %d %s" % (len(op.cols), " ".join(map(str, op.cols))))
            text = "ret rc=%d distinct=%d" % (rc, 0 if rc else len(set(op.cols)))
        elif op.kind == "set_bits":
            lines.append("set %d %s" % (len(op.cols), " ".join(str(int(c)) for c in op.cols)))
            text = "set rc=%d" % rc
        elif op.kind == "compact":
            lines.append("cmp")
            new, st = r
            text = "cmp rc=0 before=%d after=%d m=%d runs=%d nothing=%d units=%d map=%s" % (
                st["span_before"], st["span_after"], st["columns"], st["runs"], st["nothing_to_close"],
                st["units"], fold(new))
        else:
            assert op.kind == "finalize"
            lines.append("fin")
            text = "fin rc=0"
        want.append(text + " | " + state_text(m))
    return lines, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-L%d" % (c[0], c[1][0]))
def test_model_equals_the_planners(driver, sequences, case):
    lines, want = stream_and_expectation(sequences[case])
    got = driver(lines)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, lines[i], g[:300], w[:300])
    assert not any("STRAY" in g for g in got)


# ----------------------------------------------------------------------------------------------------------------------
# 2. identities
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-L%d" % (c[0], c[1][0]))
def test_model_equals_a_second_statement(sequences, case):
    seq = sequences[case]
    L = seq.shape[0]
    m = gm.GroupModel(L, seq.stride)
    ids, entry, checkpoints = {}, [], 0           # column -> identity; identity -> its expected bits

    def enter(first, columns):
        for i in range(columns.shape[1]):
            assert first + i not in ids and (not ids or first + i > max(ids))
            ids[first + i] = len(entry)
            entry.append(columns[:, i].copy())

    for step, op in enumerate(seq.ops):
        before = m.copy() if op.kind == "compact" or op.refused() else None
        r = m.apply(op)
        assert (r == op.result) if isinstance(r, int) else np.array_equal(r[0], op.result[0]) and r[1] == op.result[1], (case, step)
        if op.refused():
            assert m.same(before), (case, step, op)
            continue
        if op.kind == "add_columns":
            enter(r, np.unpackbits(op.image, axis=1, bitorder="little")[:, :op.nf].astype(bool))
        elif op.kind == "insert":
            enter(r, gm.columns_of(op.filters, L))
        elif op.kind == "retire":
            for c in set(op.cols):
                del ids[c]
        elif op.kind == "set_bits":
            for row, c in zip(np.asarray(op.rows).tolist(), np.asarray(op.cols).tolist()):
                if c in ids:
                    entry[ids[c]][row] = True
        elif op.kind == "compact":
            new, st = r
            assert all((new[c] >= 0) == (c in ids) for c in range(before.span))
            ids = {int(new[c]): i for c, i in ids.items()}
            assert st["span_before"] == before.span and st["columns"] == len(ids) and st["span_after"] == m.span == (len(ids) + 7) // 8 * 8
            if st["nothing_to_close"] or st["columns"] == 0:
                assert np.array_equal(m.matrix, before.matrix)         # nothing is launched: the memory is what it was
                assert st["units"] == 0
            else:
                assert np.array_equal(m.packed(), cc.reference(before.bits, before.real)), (case, step)
                assert not m.matrix[:, st["columns"]:(before.span + 127) // 128 * 128].any()
            assert np.array_equal(m.bits[:, :st["columns"]], before.bits[:, before.real])
        elif op.kind == "checkpoint":
            checkpoints += 1
        # at every checkpoint (and, since it costs little, after every other step too)
        real = np.flatnonzero(m.real)
        assert real.tolist() == sorted(ids) and [ids[c] for c in real.tolist()] == sorted(ids.values()), (case, step)
        assert m.num_columns == len(ids) and not m.valid[m.span:].any()
        if op.kind == "checkpoint" or step % 4 == 0:
            for c in real.tolist():
                assert np.array_equal(m.bits[:, c], entry[ids[c]]), (case, step, c)
        assert m.span == 8 * m.next_byte and m.span <= 8 * m.stride
        if m.tail_open:
            assert m.next_byte == (m.tail_column + 7) // 8 and (not real.size or real[-1] < m.tail_column)
    assert seq.ops[-1].kind == "checkpoint" and "last" in seq.ops[-1].tags
    assert checkpoints >= 3
    assert 10 <= len(seq.queries) <= 16


def test_sequences_are_deterministic():
    for case in (CASES[1], CASES[3]):
        a, b = gm.sequence(*case), gm.sequence(*case)
        assert a.queries == b.queries and [op.kind for op in a.ops] == [op.kind for op in b.ops]
        for x, y in zip(a.ops, b.ops):
            assert x.tags == y.tags
            for key in ("image", "filters", "rows", "cols", "fs"):
                assert np.array_equal(getattr(x, key, None), getattr(y, key, None))


# ----------------------------------------------------------------------------------------------------------------------
# 3. the ledger
# ----------------------------------------------------------------------------------------------------------------------

def test_ledger(sequences, oracle):
    kinds, tags, seeds_with = Counter(), Counter(), {}
    for case, seq in sequences.items():
        assert 30 <= len(seq.ops) <= 65, (case, len(seq.ops))
        for op in seq.ops:
            kinds[op.kind] += 1
            for t in op.tags:
                tags[t] += 1
                seeds_with.setdefault(t, set()).add(case[0])
        assert seq.finalizes == (case[0] % 4 != 3)
        assert any(op.search for op in seq.ops if op.kind == "checkpoint") == seq.finalizes
        pre = [op for op in seq.ops[:[i for i, op in enumerate(seq.ops) if op.kind == "checkpoint"][0]]]
        assert 2 <= sum(op.kind == "add_columns" and op.nf % 8 != 0 for op in pre) <= 3
        assert {"insert", "set_bits", "retire"} <= {op.kind for op in pre}
    for kind in ("add_columns", "insert", "retire", "set_bits", "compact", "finalize", "checkpoint"):
        assert kinds[kind] >= 10, (kind, kinds)
    for r in (0, 1, 7, 8, 31):
        assert tags["first%%32=%d" % r] >= 1, (r, tags)
    for t in ("cross1024", "cross8192", "insert_big", "insert_after_compact", "empties_unit", "retire_single", "retire_word", "retire_unit",
              "retire_last", "retire_twice", "retire_pre", "set_real", "set_retired", "set_pad", "set_any", "compact_after_insert", "compact_twice",
              "nothing_to_close", "refuse_capacity", "refuse_pad", "refuse_add", "refuse_set_at_span"):
        assert tags[t] >= 1, (t, sorted(tags.items()))
    for t in ("order1", "order2", "order3", "cache_insert", "cache_retire", "cache_compact"):
        assert len(seeds_with.get(t, ())) >= 2, (t, seeds_with.get(t))
    assert {s for s in seeds_with["order3"]} <= {c[0] for c in CASES if c[1] in gm.WIDE_SHAPES}
    # every refusal is one in the model, and the insert forms all occur
    for seq in sequences.values():
        for op in seq.ops:
            assert op.refused() == any(t.startswith("refuse_") for t in op.tags), op
    assert {op.form for seq in sequences.values() for op in seq.ops if op.kind == "insert" and not op.refused()} == set(gm.INSERT_FORMS)
    assert sum(len(op.filters) == 1 for seq in sequences.values() for op in seq.ops if op.kind == "insert") >= 10
    assert any(len(op.filters) > 1024 and not op.refused() for seq in sequences.values() for op in seq.ops if op.kind == "insert")
    # the oracle on the model at every finalizing seed's last checkpoint
    for case, seq in sequences.items():
        if not seq.finalizes:
            continue
        L, _, k, nh = seq.shape
        m = gm.GroupModel(L, seq.stride)
        for op in seq.ops:
            m.apply(op)
        assert sum(len(q) >= 300 for q in seq.queries) >= 2 and sum(len(q) < k for q in seq.queries) == 1
        counts, nk = gm.oracle_counts(oracle, m, k, nh, L, seq.queries)
        at1 = {(q, c) for q, c, _ in gm.oracle_hits(oracle, m, k, nh, L, seq.queries, 1.0)}
        at08 = {(q, c) for q, c, _ in gm.oracle_hits(oracle, m, k, nh, L, seq.queries, 0.8)}
        assert at1 and at1 <= at08, case
        assert at08 - at1, (case, "no pair passes at 0.8 only")
        hitless = [q for q in range(len(seq.queries)) if not any(h[0] == q for h in at1)]
        assert hitless, (case, "every query has a hit")
        if L >= 5:       # (a filter of one or eight rows: any column with those rows set holds every query; the query without k-mers is the one)
            assert any(nk[q] for q in hitless), (case, "every query with k-mers has a hit")
        real = np.flatnonzero(m.real)
        pairs = real[:-1][np.diff(real) == 1]
        assert (counts[:, pairs] != counts[:, pairs + 1]).any(), (case, "no neighbouring real columns differ")
        if seq.shape in gm.WIDE_SHAPES:
            # order 3 made the first long query a hit of the filled column
            assert any(q == seq.fill_query for q, _ in at1), case
