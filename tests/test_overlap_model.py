"""The numpy model of the overlap matrix (tests/overlap_model.py) against a bit-by-bit loop, and its helpers against
themselves.  No GPU, no library."""
import numpy as np
import pytest

import overlap_model as om


def random_side(rng, rows, span, dead):
    bits = rng.integers(0, 2, size=(rows, span)).astype(bool)      # the dead columns hold bits too
    valid = np.ones(span, dtype=bool)
    valid[list(dead)] = False
    return bits, valid


@pytest.mark.parametrize("rows", [1, 8, 33, 100])
def test_model_against_the_loop(rows):
    rng = np.random.default_rng(rows)
    a, va = random_side(rng, rows, 40, (3, 9))
    b, vb = random_side(rng, rows, 24, (0,))
    for ca, cb in ((None, None), ([5, 3, 5, 39, 0], [23, 0, 1]), (None, [7]), ([9], None)):
        assert np.array_equal(om.overlaps(a, va, ca, b, vb, cb), om.overlaps_loop(a, va, ca, b, vb, cb))
    sym = om.overlaps(a, va, None, a, va, None)
    assert np.array_equal(sym, sym.T) and np.array_equal(np.diag(sym), np.where(va, a.sum(axis=0), 0))
    assert not sym[3].any() and not sym[:, 9].any()
    # asymmetric where it must be
    ab = om.overlaps(a, va, [1, 2], b, vb, [4, 5, 6])
    assert ab.shape == (2, 3) and np.array_equal(om.overlaps(b, vb, [4, 5, 6], a, va, [1, 2]), ab.T)


def test_a_full_pair_wraps_to_the_cell():
    # 2^31 rows cannot be unpacked here; the wrap is the mask's: a sum of 2^32 + 5 is cell 5
    assert (np.int64((1 << 32) + 5) & 0xFFFFFFFF).astype(np.uint32) == 5
    assert np.uint32(np.int64(1 << 31) & 0xFFFFFFFF) == 0x80000000


def test_blocks_and_tiles():
    assert om.blocks_of(None, 300) == (10, 0) and om.blocks_of(None, 0) == (0, 0)
    assert om.blocks_of(list(range(64, 128)), 300) == (2, 0)
    assert om.blocks_of(list(range(65, 129)), 300) == (0, 2)
    assert om.blocks_of(list(range(64, 127)), 300) == (1, 1)            # a short last block is gathered
    assert om.blocks_of(list(range(32)) + [40] + list(range(32, 64)), 300) == (1, 2)
    assert om.tiles_of(300, 300, True) == 6 and om.tiles_of(300, 129, False) == 6 and om.tiles_of(128, 128, True) == 1


@pytest.mark.parametrize("kind", om.LIST_KINDS)
def test_lists_name_live_columns(kind):
    rng = np.random.default_rng(3)
    valid = np.ones(440, dtype=bool)
    valid[[5, 77, 78, 130, 300]] = False
    cols = om.list_of(rng, kind, valid)
    assert valid[cols].all() and len(cols) >= 9
    s, g = om.blocks_of(cols, 440)
    assert (s > 0) == (kind in ("aligned", "mixed")) and (g > 0) == (kind != "aligned")
    if kind == "repeat":
        assert len(set(cols.tolist())) < len(cols)
