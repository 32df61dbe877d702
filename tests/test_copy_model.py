"""The sequences of tests/copy_model.py checked without a device: they are deterministic, at most 40 steps long, every
seed holds at least three successful copies in each direction and at most a quarter of its copy steps are refusals, the
kinds of lists and refusals all occur across the seeds, and after every successful copy the destination model holds the
source model's listed columns at the place a live insert would have taken -- a second statement in numpy, beside the
model's own insert."""
from collections import Counter

import numpy as np

import copy_model as cm
import group_model as gm


def test_sequences_are_deterministic_and_short():
    for seed in cm.SEEDS[:3]:
        a, b = cm.sequence(seed), cm.sequence(seed)
        assert len(a) == len(b) <= cm.MAX_STEPS
        for x, y in zip(a, b):
            assert (x.kind, x.on, sorted(x.tags)) == (y.kind, y.on, sorted(y.tags))
            assert (x.result == y.result) if isinstance(x.result, int) else np.array_equal(x.result[0], y.result[0])
    assert all(len(cm.sequence(seed)) <= cm.MAX_STEPS for seed in cm.SEEDS)


def test_every_seed_copies_both_ways_and_refusals_stay_a_quarter():
    kinds = Counter()
    for seed in cm.SEEDS:
        ops = cm.sequence(seed)
        copies = [op for op in ops if op.kind == "copy"]
        good = [op for op in copies if not op.refused()]
        for way in ("AB", "BA"):
            assert sum(way in op.tags for op in good) >= 3, (seed, way)
        assert 4 * (len(copies) - len(good)) <= len(copies), (seed, len(copies), len(good))
        assert sum(op.kind == "finalize" for op in ops) == 1 and any(op.kind == "compact" for op in ops)
        assert any(op.kind == "retire" for op in ops) and any(op.kind == "set_bits" for op in ops) and any(op.kind == "insert" for op in ops)
        kinds.update(t for op in copies for t in op.tags if t.startswith(("copy_", "refuse_")))
    assert all(kinds["copy_" + how] for how in ("all", "ascending", "reversed", "shuffled", "one")), kinds
    assert all(kinds["refuse_" + how] for how in ("twice", "beyond", "same", "empty", "pad")), kinds


def test_a_copy_is_the_insert_of_the_sources_columns():
    offsets = Counter()
    for seed in cm.SEEDS:
        models = cm.fresh_models()
        for step, op in enumerate(cm.sequence(seed)):
            before = {name: m.copy() for name, m in models.items()}
            got = cm.apply(models, op)
            if op.kind != "copy":
                continue
            assert got == op.result, (seed, step)
            dst, src = models[op.on], before[op.src]
            assert models[op.src].same(before[op.src]) or op.src == op.on, (seed, step)
            if op.refused():
                assert dst.same(before[op.on]), (seed, step)
                continue
            old = before[op.on]
            cols = np.flatnonzero(src.real) if op.cols is None else np.asarray(op.cols)
            first, n = got, cols.size
            assert first == (old.tail_column if old.tail_open else (old.next_byte + 15) // 16 * 16 * 8), (seed, step)
            word_end = ((first + n - 1) // 32 + 1) * 32
            want = old.matrix.copy()
            want[:, first:first + n] = src.matrix[:, cols]
            want[:, first + n:word_end] = False
            assert np.array_equal(dst.matrix, want), (seed, step)
            assert np.array_equal(np.flatnonzero(dst.valid), np.union1d(np.flatnonzero(old.valid), np.arange(first, first + n)))
            assert (dst.tail_open, dst.tail_column, dst.next_byte, dst.finalized) == (True, first + n, (first + n + 7) // 8, old.finalized)
            offsets[first % 32 != 0] += 1
    assert offsets[True] >= 10 and offsets[False] >= 3, offsets
