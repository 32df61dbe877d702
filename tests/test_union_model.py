"""tests/union_model.py held to itself, without a device: the model of the union against a bit-by-bit restatement on every
case of the table, the placement rules (the live insert's between two groups, the next 16-byte boundary within one), the
refusals, and the table's coverage -- every filter length with every list, every destination state, every source."""
import numpy as np
import pytest

import group_model as gm
import union_model as um


def replay(case):
    ops, dst_name, caps, rng = um.case_ops(case)
    models = um.fresh_models(case, caps)
    for op in ops:
        r = models[op.on].apply(op)
        assert not (isinstance(r, int) and r < 0), (case, op)
    return models, dst_name, um.lists_of(rng, case[3], models["S"])


@pytest.fixture(scope="module")
def replayed():
    return {case: replay(case) for case in um.CASES}


def test_the_table_covers_what_it_promises(replayed):
    assert len(set(um.CASES)) == len(um.CASES)
    assert {(c[0], c[3]) for c in um.CASES} >= {(L, lst) for L in um.LS for lst in um.LISTS}
    assert {c[2] for c in um.CASES} == set(um.DESTS) and {c[1] for c in um.CASES} == set(um.SOURCES)
    assert {(c[2], c[3]) for c in um.CASES} >= {(d, lst) for d in um.DESTS for lst in ("129sets", "unequal")}
    firsts, units, keeps_high = set(), set(), 0
    for case, (models, dst_name, sets) in replayed.items():
        dst, src = models[dst_name], models["S"]
        first = dst.tail_column if dst.tail_open and dst is not src else (dst.next_byte + 15) // 16 * 16 * 8
        firsts.add(first % 128)
        units.add((first + len(sets) + 127) // 128 - first // 128)
        word_end = ((first + len(sets) - 1) // 32 + 1) * 32
        keeps_high += bool(dst.matrix[:, word_end:(word_end + 127) // 128 * 128].any())
        if case[1] == "retired":                      # bits left in a retired column beside a member, bits in a pad column
            assert src.matrix[:, 33].all() and not src.valid[33] and src.valid[34]
            assert case[2] in ("same-open", "same-final") or (src.matrix[:, 71].any() and not src.valid[71])      # (there an insert took the pad)
        if case[1] == "blocks":                       # garbage in the pad bits of a file block
            assert src.matrix[:, 77:80].any() and not src.valid[77:80].any()
        if case[1] == "kib":
            assert src.span > 8192 and src.valid[8191] and src.valid[8192]
        if case[3] == "200sets":
            assert len(sets) == 200 and all(sets[0][0] in s for s in sets)
        if case[3] == "repeat":
            assert any(len(s) != len(set(s)) for s in sets)
        if case[3] == "dwords":
            assert len({c // 32 for c in sets[0]}) == 1 and len({c // 32 for c in sets[1]}) == 2
            assert sets[2] == [int(np.flatnonzero(src.real)[0]), int(np.flatnonzero(src.real)[-1])]
    assert firsts >= {0, 1, 31, 32, 33, 127} and units >= {1, 2, 3} and keeps_high >= 1


@pytest.mark.parametrize("case", um.CASES, ids=um.case_id)
def test_the_model_is_the_or_of_the_members(replayed, case):
    models, dst_name, sets = replayed[case]
    models = {name: m.copy() for name, m in models.items()}
    dst, src = models[dst_name], models["S"]
    before, src_before = dst.copy(), src.copy()
    first = um.union(dst, src, sets)
    n = len(sets)
    # the place
    if dst is src:
        assert first == (before.next_byte + 15) // 16 * 16 * 8 and first % 128 == 0 and first >= before.span
    else:
        assert first == (before.tail_column if before.tail_open else (before.next_byte + 15) // 16 * 16 * 8)
        assert src.same(src_before)
    # the state: the live insert's
    assert (dst.tail_open, dst.tail_column, dst.next_byte, dst.finalized) == (True, first + n, (first + n + 7) // 8, before.finalized)
    assert dst.num_columns == before.num_columns + n and dst.valid[first:first + n].all()
    assert np.array_equal(dst.valid[:first], before.valid[:first]) and not dst.valid[first + n:].any()
    # the bits, one by one: a new column's bit is set where any member's is; everything below `first` is kept, zero from the
    # new tail to the end of its 32-bit word, everything above that kept
    word_end = ((first + n - 1) // 32 + 1) * 32
    assert np.array_equal(dst.matrix[:, :first], before.matrix[:, :first])
    assert not dst.matrix[:, first + n:word_end].any() and np.array_equal(dst.matrix[:, word_end:], before.matrix[:, word_end:])
    rows = range(dst.nrows) if dst.nrows <= 64 else range(0, dst.nrows, 37)
    for j in sorted({0, 1, n // 2, n - 1} & set(range(n))):
        for r in rows:
            want = False
            for c in sets[j]:
                want = want or bool(src_before.matrix[r, c])
            assert bool(dst.matrix[r, first + j]) == want, (j, r)
    # a set of one member is a copy of that column
    for j, s in enumerate(sets):
        if len(set(s)) == 1:
            assert np.array_equal(dst.matrix[:, first + j], src_before.matrix[:, s[0]])


def test_the_model_refuses_what_the_call_refuses():
    rng = np.random.default_rng(5)
    src, dst, short = gm.GroupModel(5, 128), gm.GroupModel(5, 128), gm.GroupModel(4, 128)
    src.insert(gm.random_filters(rng, 5, 40))
    src.retire([7])
    dst.insert(gm.random_filters(rng, 5, 1000))
    states = src.copy(), dst.copy()
    for sets in ([], [[1], []], [[1, 40]], [[1], [7]], [[1, 100000]]):
        assert um.union(dst, src, sets) == um.ERR_ARG and um.union(src, src, sets) == um.ERR_ARG
    assert um.union(short, src, [[1]]) == um.ERR_ARG
    assert um.union(dst, src, [[1]] * 25) == um.ERR_ARG          # capacity: 1000 + 25 > 1024
    assert um.union(src, src, [[1]] * 897) == um.ERR_ARG         # within one group: 128 + 897 > 1024 behind the pad
    assert src.same(states[0]) and dst.same(states[1])
    assert um.union(dst, src, [[1]] * 24) == 1000 and um.union(src, src, [[1]] * 896) == 128
