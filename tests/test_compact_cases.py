"""The table of the compaction's cases (tests/compact_cases.py) checked on its own, without a device: each case really has
the edge it is there for, the residues of m are the ones asked for, and the numpy reference is what the issue states --
np.packbits(image[:, valid], axis=1, bitorder="little") with new_column the rank among the valid columns."""
import numpy as np
import pytest

import compact_cases as cc

BY_NAME = {c.name: c for c in cc.CASES}


def sizings(case):
    return [cc.sized(case, r) for r in cc.RESIDUES] if case.grow is not None else [case]


def test_the_table_names_every_case_once():
    assert [c.name for c in cc.CASES] == list("abcdefghij")
    assert BY_NAME["a"].blocks == BY_NAME["b"].blocks == BY_NAME["c"].blocks == [70000]
    assert BY_NAME["i"].blocks == [70, 1, 300] and BY_NAME["j"].inserts == [5, 3] and BY_NAME["j"].after == 4


@pytest.mark.parametrize("name", "abcdefgj")
def test_residues(name):
    for r, c in zip(cc.RESIDUES, sizings(BY_NAME[name])):
        lay = cc.layout(c)
        assert lay.m % cc.UNIT == r
        assert 0 <= c.blocks[c.grow] - BY_NAME[name].blocks[c.grow] < cc.UNIT
    assert cc.layout(sizings(BY_NAME[name])[1]).m % 8 != 0


def test_fixed_cases():
    assert cc.layout(BY_NAME["h"]).m == 0 and cc.layout(BY_NAME["i"]).m == 371 and 371 % 8 != 0


@pytest.mark.parametrize("case", [s for c in cc.CASES for s in sizings(c)], ids=lambda c: "%s-%d" % (c.name, sum(c.blocks)))
def test_each_case_has_its_edge(case):
    lay = cc.layout(case)
    pl = cc.plan(lay)
    src = np.flatnonzero(lay.valid)                 # source column of destination column d
    shift = src - np.arange(src.size)
    lanes, rows_per_wg, segments = cc.schedule(pl["units"])
    assert np.all(shift >= 0)                       # the rule in-place rests on
    assert pl["columns"] == lay.m == len(lay.columns) - len(lay.retired) and pl["span_after"] % 8 == 0
    if case.name in "abc":
        assert lay.span == 8 * ((sum(case.blocks) + 7) // 8) and lanes == cc.SEGMENT and rows_per_wg == 1
    if case.name == "a":
        assert pl["runs"] == 1 and np.all(shift == 1) and pl["first_unit"] == 0 and segments >= 3
        # every store of a segment but the last unit's hits the next thread's source: only the barrier orders them
    elif case.name == "b":
        assert pl["runs"] == 1 and shift[0] == 33005 > cc.SEGMENT * cc.UNIT and segments >= 3
    elif case.name == "c":
        assert pl["first_unit"] == 40000 // cc.UNIT > cc.SEGMENT and np.all(shift[:40000] == 0) and pl["runs"] == 2
        assert segments == 1                        # (what is left of the row is less than a segment)
    elif case.name == "d":
        runs_of_one = np.count_nonzero(np.diff(src[999:1256]) == 2)
        assert runs_of_one >= 255 and pl["runs"] == 257 and pl["first_unit"] == 1000 // cc.UNIT
    elif case.name == "e":
        assert pl["runs"] == 3 and set(np.unique(shift)) == {0, 128, 128 + 1024} and pl["first_unit"] == 1
    elif case.name == "f":
        assert lay.retired == [31, 32, 127, 128, 129] and pl["runs"] == 3 and pl["first_unit"] == 0
    elif case.name == "g":
        assert np.all(shift == 0) and pl["runs"] == 1 and pl["span_after"] < pl["span_before"] and pl["units"] >= 1
        assert pl["first_unit"] == lay.m // cc.UNIT
    elif case.name == "h":
        assert lay.m == 0 and pl["runs"] == 0 and pl["units"] == 0 and pl["span_after"] == 0
    elif case.name == "i":
        assert not lay.retired and pl["runs"] == 3 and lay.span == 560 and lay.capacity <= 1024      # a row of 128 bytes
        assert (lanes, rows_per_wg, segments) == (8, 32, 1) and pl["first_unit"] == 0 and pl["units"] == 5
    elif case.name == "j":
        assert lay.tail is not None and len(lay.retired) == 1 and lay.retired[0] == lay.columns[-6]
        assert lay.m + case.after <= lay.capacity and pl["runs"] == 4      # two blocks, the insert cut in two


def test_the_reference_is_packbits_of_the_valid_columns_and_the_map_is_the_rank():
    case = BY_NAME["f"]
    lay = cc.layout(case)
    img = cc.image(case, 16)
    ref = cc.reference(img, lay.valid)
    assert np.array_equal(ref, np.packbits(img[:, lay.valid], axis=1, bitorder="little"))
    assert ref.shape == (16, (lay.m + 7) // 8)
    # bit by bit: destination column d of a row is the d-th valid source column; the pad bits of the last byte are zero
    bits = np.unpackbits(ref, axis=1, bitorder="little")
    src = np.flatnonzero(lay.valid)
    for d in (0, 30, 31, 32, 125, 126, 127, 128, lay.m - 1):
        assert np.array_equal(bits[:, d], img[:, src[d]]) and lay.new_column[src[d]] == d
    assert not bits[:, lay.m:].any()
    assert all(lay.new_column[c] == -1 for c in lay.retired)
    rank = [int(lay.valid[:c].sum()) if lay.valid[c] else -1 for c in range(0, lay.span, 97)]
    assert rank == lay.new_column[::97].tolist()
    assert img[:, lay.retired].any()                # (the image holds bits there: the tests retire them on the device)
