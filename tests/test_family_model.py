"""The family of tests/family_model.py and its walks, checked without a device -- every sequence that
tests/test_gpu_family_model.py replays on the GPU is inspected here first.

  1. the walks are deterministic, at most 60 steps long, and never have more than five groups alive;
  2. a second statement of the fold: after every successful fold the new model's packed rows are a plain loop
     dst[r % 2^L2] |= src[r] over bytes [0, 16 U), zero above, the layout the source's, the source and every other model as
     before; after every refused step every model is as before;
  3. the meaning of the fold, by identities as tests/test_group_model.py keeps them: every column gets an identity when it
     enters (the sample it is the exact filter of, or its entry bits, and what set_bits planted in it while it was real);
     folds, copies and compactions carry identities along, and every real column of every group must equal
     oracle.bloom_bits_from_sequences([sample], k, nh, L of ITS group) -- for a column that was folded, the filter at the
     short length -- OR-ed with the planted bits folded by the plain rule;
  4. the family against the library's own planners: tests/sanitize/family_model_driver.cpp, built with
     g++ -fsanitize=address,undefined as a stand-alone program, runs fold_refusal / plan_fold, copy_refusal / plan_copy /
     plan_insert and the planners of the single-group driver on every default walk; every line equals what the model says;
  5. a ledger: every order and refusal kind family_model names occurs in at least two seeds, refusals stay a quarter of a
     seed's fold and copy steps, and the CPU oracle finds on the fold's model, at each finalizing seed's last checkpoint, a
     hit at t = 1, a pair that passes at 0.8 only and a query with k-mers and no hit.
Nothing of the library is loaded into python."""
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT

import family_model as fm
import group_model as gm

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")
SEEDS = fm.default_seeds(max(int(os.environ.get("KWAGE_MODEL_SEEDS", "12")), 12))


@pytest.fixture(scope="module")
def sequences():
    return {seed: fm.sequence(seed) for seed in SEEDS}


def results_equal(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and np.array_equal(a[0], b[0]) and a[1] == b[1]
    return a == b


# ----------------------------------------------------------------------------------------------------------------------
# 1. determinism and length
# ----------------------------------------------------------------------------------------------------------------------

def test_walks_are_deterministic_short_and_small(sequences):
    for seed in (SEEDS[0], SEEDS[1], SEEDS[4]):
        a, b = sequences[seed], fm.sequence(seed)
        assert a.queries == b.queries and len(a.ops) == len(b.ops)
        for x, y in zip(a.ops, b.ops):
            assert (x.kind, x.on, x.tags) == (y.kind, y.on, y.tags) and results_equal(x.result, y.result)
            for key in ("image", "filters", "rows", "cols", "fs", "src", "L2", "L"):
                assert np.array_equal(getattr(x, key, None), getattr(y, key, None))
    for seed, seq in sequences.items():
        assert 25 <= len(seq.ops) <= fm.MAX_STEPS, (seed, len(seq.ops))
        assert seq.shape == (fm.WIDE if seed % 3 == 0 else fm.NARROW)
        fam = fm.Family(seq.shape)
        for op in seq.ops:
            fam.apply(op)
            assert 1 <= len(fam.models) <= fm.MAX_ALIVE, (seed, op)
        assert seq.ops[-1].kind == "checkpoint" and "last" in seq.ops[-1].tags and 10 <= len(seq.queries) <= 16


# ----------------------------------------------------------------------------------------------------------------------
# 2. and 3. a second statement of the fold, and its meaning
# ----------------------------------------------------------------------------------------------------------------------

class Identity:
    """What a column must hold: the exact filter of sample `genome` at the length of the group it stands in (or, for a
    column that entered as bits, `entry`), OR `planted`; both bool [rows of its group]."""

    def __init__(self, genome, entry, nrows):
        self.genome, self.entry, self.planted = genome, entry, np.zeros(nrows, dtype=bool)

    def folded(self, L2):
        def fold(bits):
            out = np.zeros(1 << L2, dtype=bool)
            for r in np.flatnonzero(bits):
                out[r % (1 << L2)] = True
            return out
        i = Identity(self.genome, None if self.entry is None else fold(self.entry), 1 << L2)
        i.planted = fold(self.planted)
        return i

    def clone(self):
        i = Identity(self.genome, None if self.entry is None else self.entry.copy(), self.planted.size)
        i.planted = self.planted.copy()
        return i


@pytest.mark.parametrize("seed", SEEDS)
def test_family_equals_a_second_statement(sequences, oracle, seed):
    seq = sequences[seed]
    _, _, k, nh = seq.shape
    fam = fm.Family(seq.shape)
    ids = {}                                            # group -> {column: Identity}
    exact = {}                                          # (sample, L) -> bool [2^L]
    folded_genomes = 0

    def expected(i, L):
        if i.genome is None:
            return i.entry | i.planted
        if (i.genome, L) not in exact:
            exact[(i.genome, L)] = gm.columns_of(oracle.bloom_bits_from_sequences([seq_genomes[i.genome]], k, nh, L)[None, :], L)[:, 0]
        return exact[(i.genome, L)] | i.planted

    seq_genomes = seq.genomes
    for step, op in enumerate(seq.ops):
        what = (seed, step, op)
        before = fam.copy()
        r = fam.apply(op)
        assert results_equal(r, op.result), what
        if op.refused():
            assert fam.same(before), what
            continue
        # every model the step does not name is as before
        named = {op.on}
        for name, m in fam.models.items():
            if name not in named:
                assert m.same(before.models[name]), (what, name)
        m = fam.models.get(op.on)
        if op.kind == "new":
            assert m.L == op.L and m.span == 0 and not m.matrix.any() and not m.valid.any() and not m.finalized and m.stride == seq.stride
            ids[op.on] = {}
        elif op.kind == "close":
            del ids[op.on]
        elif op.kind == "fold":
            src = before.models[op.src]
            units = (src.next_byte + 15) // 16
            packed = np.packbits(src.matrix, axis=1, bitorder="little")
            want = np.zeros((1 << op.L2, src.stride), dtype=np.uint8)
            want[:, :16 * units] = fm.fold_rows(packed[:, :16 * units], op.L2)
            assert np.array_equal(np.packbits(m.matrix, axis=1, bitorder="little"), want), what
            assert (m.L, m.stride, m.next_byte, m.tail_open, m.tail_column, m.finalized) == (op.L2, src.stride, src.next_byte, src.tail_open, src.tail_column, src.finalized)
            assert np.array_equal(m.valid, src.valid)
            assert r == {"log_2_before": src.L, "log_2_after": op.L2, "units_per_row": units, "bytes_read": src.nrows * units * 16,
                         "bytes_written": m.nrows * units * 16}, what
            ids[op.on] = {c: i.folded(op.L2) for c, i in ids[op.src].items()}
            folded_genomes += sum(i.genome is not None for i in ids[op.on].values())
            if hasattr(op, "twin"):
                assert m.same(fam.models[op.twin]) and m.L == fam.models[op.twin].L, what
        elif op.kind == "add_columns":
            cols = np.unpackbits(op.image, axis=1, bitorder="little")[:, :op.nf].astype(bool)
            for j in range(op.nf):
                ids[op.on][r + j] = Identity(None, cols[:, j].copy(), m.nrows)
        elif op.kind == "insert":
            cols = gm.columns_of(op.filters, m.L)
            for j, g in enumerate(op.genomes):
                ids[op.on][r + j] = Identity(g if g >= 0 else None, None if g >= 0 else cols[:, j].copy(), m.nrows)
        elif op.kind == "copy":
            src = ids[op.src]
            cols = sorted(src) if op.cols is None else list(op.cols)
            for j, c in enumerate(cols):
                ids[op.on][r + j] = src[c].clone()
        elif op.kind == "retire":
            for c in set(op.cols):
                del ids[op.on][c]
        elif op.kind == "set_bits":
            for row, c in zip(np.asarray(op.rows).tolist(), np.asarray(op.cols).tolist()):
                if c in ids[op.on]:
                    ids[op.on][c].planted[row] = True
        elif op.kind == "compact":
            new = r[0]
            ids[op.on] = {int(new[c]): i for c, i in ids[op.on].items()}
        # every real column of every group is what its identity says
        for name, gmodel in fam.models.items():
            assert np.flatnonzero(gmodel.real).tolist() == sorted(ids[name]) and not gmodel.valid[gmodel.span:].any(), (what, name)
            assert gmodel.span == 8 * gmodel.next_byte <= 8 * gmodel.stride
            if name in named or op.kind == "checkpoint":
                for c, i in ids[name].items():
                    assert np.array_equal(gmodel.matrix[:, c], expected(i, gmodel.L)), (what, name, c)
    assert folded_genomes >= 12, (seed, folded_genomes)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the planners
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("family_model")
    exe = str(tmp / "family_model_driver")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "family_model_driver.cpp"), "-o", exe, "-lz", "-lpthread"]
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


def state_text(m):
    return "L=%d span=%d open=%d tail=%d columns=%d final=%d valid=%s" % (m.L, m.span, m.tail_open, m.tail_column, m.num_columns, m.finalized,
                                                                          np.packbits(m.real, bitorder="little").tobytes().hex())


def stream_and_expectation(seq):
    """(the driver's input, the lines the model says it must print) for one walk."""
    fam = fm.Family(seq.shape)
    lines, want = [], []
    for op in seq.ops:
        if op.kind == "checkpoint":
            continue
        src_before = fam.models[op.src].copy() if op.kind == "copy" else None
        r = fam.apply(op)
        rc = r if isinstance(r, int) and r < 0 else 0
        shown = fam.models.get(op.on)
        if op.kind == "new":
            lines.append("new %s %d %d" % (op.on, op.L, seq.stride))
            text = "new rc=0"
        elif op.kind == "close":
            lines.append("close %s" % op.on)
            want.append("close rc=0")
            continue
        elif op.kind == "fold":
            lines.append("fold %s %d %s" % (op.src, op.L2, op.on))
            text = "fold rc=%d units=%d read=%d written=%d" % ((rc, 0, 0, 0) if rc else (0, r["units_per_row"], r["bytes_read"], r["bytes_written"]))
            shown = fam.models[op.src] if rc else shown
        elif op.kind == "copy":
            lines.append("copy %s %s %s" % (op.on, op.src, "-1" if op.cols is None else " ".join(map(str, [len(op.cols)] + list(op.cols)))))
            if rc:
                text = "copy rc=%d first=0 runs=0 first_unit=0 units=0" % rc
            else:
                cols = np.flatnonzero(src_before.real) if op.cols is None else np.asarray(op.cols)
                runs = 1 + int(np.count_nonzero(np.diff(cols) != 1))
                text = "copy rc=0 first=%d runs=%d first_unit=%d units=%d" % (r, runs, r // 128, (r + cols.size + 127) // 128 - r // 128)
        elif op.kind == "add_columns":
            lines.append("add %s %d" % (op.on, op.nf))
            text = "add rc=%d first=%d" % (rc, 0 if rc else r)
        elif op.kind == "insert":
            n = len(op.filters)
            lines.append("ins %s %d" % (op.on, n))
            text = "ins rc=%d first=%d word_first=%d word_last=%d keep=%d" % ((rc, 0, 0, 0, 0) if rc else (0, r, r // 32, (r + n - 1) // 32, r % 32))
        elif op.kind == "retire":
            lines.append("ret %s %d %s" % (op.on, len(op.cols), " ".join(map(str, op.cols))))
            text = "ret rc=%d distinct=%d" % (rc, 0 if rc else len(set(op.cols)))
        elif op.kind == "set_bits":
            lines.append("set %s %d %s" % (op.on, len(op.cols), " ".join(str(int(c)) for c in op.cols)))
            text = "set rc=%d" % rc
        elif op.kind == "compact":
            lines.append("cmp %s" % op.on)
            st = r[1]
            text = "cmp rc=0 before=%d after=%d m=%d runs=%d nothing=%d units=%d" % (st["span_before"], st["span_after"], st["columns"], st["runs"],
                                                                                   st["nothing_to_close"], st["units"])
        else:
            assert op.kind == "finalize"
            lines.append("fin %s" % op.on)
            text = "fin rc=0"
        want.append(text + " | " + state_text(shown))
    return lines, want


@pytest.mark.parametrize("seed", SEEDS)
def test_family_equals_the_planners(driver, sequences, seed):
    lines, want = stream_and_expectation(sequences[seed])
    got = driver(lines)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (seed, i, lines[i], g[:300], w[:300])
    assert not any("STRAY" in g for g in got)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the ledger
# ----------------------------------------------------------------------------------------------------------------------

def test_ledger(sequences, oracle):
    default = {seed: seq for seed, seq in sequences.items() if seed < 12}
    seeds_with, lists = {}, Counter()
    residues = set()
    for seed, seq in default.items():
        for op in seq.ops:
            for t in op.tags:
                seeds_with.setdefault(t, set()).add(seed)
        folds = [op for op in seq.ops if op.kind == "fold"]
        copies = [op for op in seq.ops if op.kind == "copy"]
        good_folds = [op for op in folds if not op.refused()]
        good_copies = [op for op in copies if not op.refused() and op.tags & {"copy_from_fold", "copy_into_fold"}]
        assert len(good_folds) >= 2 and len(good_copies) >= 3, (seed, len(good_folds), len(good_copies))
        refused = sum(op.refused() for op in folds + copies)
        assert refused >= 1 and 4 * refused <= len(folds) + len(copies), (seed, refused, len(folds) + len(copies))
        assert sum(t in fm.ORDERS for op in seq.ops for t in op.tags) >= 4, seed          # (several orders in every seed)
        assert seq.finalizes == (seed % 4 != 3)
        searched = [op for op in seq.ops if op.kind == "checkpoint" and op.search]
        assert bool(searched) == seq.finalizes and (not seq.finalizes or any("on_fold" in op.tags for op in searched)), seed
        for i, op in enumerate(seq.ops):
            assert op.refused() == any(t.startswith("refuse_") for t in op.tags), (seed, op)
            if op.kind == "insert" and "into_fold" in op.tags:
                residues.add(op.result % 32)
            if op.kind == "copy" and not op.refused():
                lists.update(t for t in op.tags if t.startswith("copy_") or t in ("dst_final", "dst_open", "src_final", "src_open"))
            if "fold_final" in op.tags:            # the fold of a finalized group: searched at once, add_columns refused, an insert taken
                nxt = [o for o in seq.ops[i + 1:] if o.kind != "close"][0]
                assert nxt.kind == "checkpoint" and nxt.on == op.on and nxt.search and "after_fold_final" in nxt.tags
                rest = [o for o in seq.ops[i + 1:] if o.on == op.on]
                assert any(o.kind == "add_columns" and o.result == fm.ERR_STATE for o in rest) and any(o.kind == "insert" and not o.refused() for o in rest)
            if "fold_open" in op.tags:
                rest = [o for o in seq.ops[i + 1:] if o.on == op.on]
                assert rest[0].kind == "add_columns" and not rest[0].refused()
                assert any(o.kind == "finalize" for o in rest) == seq.finalizes
            if "fold_then_close_src" in op.tags:
                assert seq.ops[i + 1].kind == "close" and seq.ops[i + 1].on == op.src
                assert sum(o.on == op.on and o.kind in ("insert", "copy", "compact", "set_bits", "retire") for o in seq.ops[i + 2:]) >= 5
            if "fold_open_tail" in op.tags:
                a, b = seq.ops[i + 1], seq.ops[i + 2]
                assert (a.kind, a.on, b.kind, b.on) == ("insert", op.on, "insert", op.src) and a.result == b.result and a.result % 32 in fm.RESIDUES
    for t in fm.ORDERS + tuple("refuse_" + r for r in fm.REFUSALS):
        assert len(seeds_with.get(t, ())) >= 2, (t, seeds_with.get(t))
    assert {"fold_final", "after_fold_final"} <= {t for t in seeds_with if seeds_with[t] & {s for s in default if s % 3 == 0}}      # (on a wide seed)
    assert residues >= {0, 1, 7, 8, 31}, residues
    for t in ["copy_" + how for how in fm.COPY_LISTS] + ["dst_final", "dst_open", "src_final", "src_open"]:
        assert lists[t] >= 2, (t, lists)
    for L2 in (10, 7, 6, 5, 3, 0):
        assert seeds_with.get("to%d" % L2), L2
    # the oracle on the fold's model at every finalizing seed's last checkpoint
    for seed, seq in default.items():
        if not seq.finalizes:
            continue
        _, _, k, nh = seq.shape
        fam = fm.Family(seq.shape)
        for op in seq.ops:
            fam.apply(op)
        last = seq.ops[-1]
        m = fam.models[last.on]
        assert "on_fold" in last.tags and last.search and m.finalized
        assert sum(len(q) >= 300 for q in seq.queries) >= 2 and sum(len(q) < k for q in seq.queries) == 1
        _, nk = gm.oracle_counts(oracle, m, k, nh, m.L, seq.queries)
        at1 = {(q, c) for q, c, _ in gm.oracle_hits(oracle, m, k, nh, m.L, seq.queries, 1.0)}
        at08 = {(q, c) for q, c, _ in gm.oracle_hits(oracle, m, k, nh, m.L, seq.queries, 0.8)}
        assert at1 and at1 <= at08, seed
        assert at08 - at1, (seed, "no pair passes at 0.8 only")
        hitless = [q for q in range(len(seq.queries)) if not any(h[0] == q for h in at1)]
        assert any(nk[q] for q in hitless), (seed, "every query with k-mers has a hit")
