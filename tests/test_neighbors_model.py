"""tests/neighbors_model.py against a bit-by-bit loop on tiny cases, and the claim the device's scalar Jaccard key rests
on: floor(s 2^64 / u) orders fractions exactly as the fractions order themselves."""
from fractions import Fraction

import numpy as np
import pytest

import neighbors_model as nm
import overlap_model as om


class Tiny:
    """What neighbors_model.of_models reads of a group model."""

    def __init__(self, rng, rows, span, dead=()):
        self.bits = rng.random((rows, span + 3)) < 0.4
        self.real = np.ones(span, dtype=bool)
        self.real[list(dead)] = False
        self.span, self.nrows = span, rows


@pytest.mark.parametrize("metric", [nm.SHARED, nm.JACCARD])
@pytest.mark.parametrize("rows", [1, 7, 40])
def test_the_model_against_a_loop(metric, rows):
    rng = np.random.default_rng(rows)
    a, b = Tiny(rng, rows, 9, dead=[2]), Tiny(rng, rows, 6, dead=[0, 5])
    a.bits[:, 4] = a.bits[:, 3]                                 # an identical pair
    a.bits[:, 7] = False                                        # an empty column
    for k in (1, 3, 20):
        for min_shared in (0, 2):
            for cols_a, other, cols_b, skip in ((None, None, None, True), (None, None, None, False), ([3, 4, 3, 8, 1], None, None, True),
                                                ([1, 3], a, None, True), ([8, 0, 4], b, [4, 1, 1, 2], True), (None, b, None, False)):
                got = nm.of_models(a, cols_a, other, cols_b, k, metric, min_shared, skip)
                la = list(range(a.span)) if cols_a is None else cols_a
                mb = a if other is None else other
                lb = la if other is None else list(range(mb.span)) if cols_b is None else cols_b
                want = nm.select_loop(a.bits, a.real, la, mb.bits, mb.real, lb, k, metric, min_shared, skip and mb is a)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, min_shared, cols_a, cols_b)
                assert (got[0][got[0][:, :, 0] == 0xFFFFFFFF] == nm.FILLER).all()


def test_dead_entries_and_filler():
    rng = np.random.default_rng(1)
    a = Tiny(rng, 16, 5, dead=[1])
    rec, cnt = nm.of_models(a, None, None, None, 6, nm.JACCARD, skip_self=True)
    assert cnt.tolist() == [3, 0, 3, 3, 3] and (rec[1] == nm.FILLER).all() and (rec[:, 3:] == nm.FILLER).all()
    assert not (rec[:, :3, 0][cnt > 0] == 1).any()
    rec, cnt = nm.of_models(a, None, None, None, 2, nm.SHARED)
    assert (rec[[0, 2, 3, 4], 0, 0] == [0, 2, 3, 4]).all()      # a column shares most with itself


def test_the_key_orders_every_small_fraction():
    pairs = [(s, u) for u in range(65) for s in range(u + 1)]
    keys = {p: nm.device_key(*p) for p in pairs}
    frac = {p: (Fraction(p[0], p[1]) if p[1] else Fraction(0)) for p in pairs}
    for p in pairs:
        assert 0 <= keys[p] < 1 << 64
        for q in pairs:
            assert (keys[p] > keys[q]) == (frac[p] > frac[q]) and (keys[p] == keys[q]) == (frac[p] == frac[q]), (p, q)


def test_the_key_orders_fractions_with_denominators_near_2_32():
    rng = np.random.default_rng(32)
    top = 1 << 32
    us = [top, top - 1, top - 2, top - 3] + [int(top - x) for x in rng.integers(0, 1 << 20, 60)]
    pairs = []
    for u in us:
        for s in [0, 1, u - 1, u, u // 2, u // 2 + 1] + [int(x) for x in rng.integers(0, u, 6)]:
            if s <= min(u, 1 << 31) or s == u:
                pairs.append((s, u))
    # neighbours in the Farey sense: s / u against (s + 1) / (u + 1) and s / (u - 1), the closest pairs there are
    for s, u in list(pairs):
        if u < top and s < u:
            pairs.append((s + 1, u + 1))
        if s < u - 1:
            pairs.append((s, u - 1))
    keys = [nm.device_key(s, u) for s, u in pairs]
    frac = [Fraction(s, u) for s, u in pairs]
    order = sorted(range(len(pairs)), key=lambda i: frac[i])
    for x, y in zip(order, order[1:]):
        assert (keys[x] < keys[y]) == (frac[x] < frac[y]) and (keys[x] == keys[y]) == (frac[x] == frac[y]), (pairs[x], pairs[y])
    # the planted pair of the device test: 1e-8 apart, equal as float32
    a, b = (5000, 10001), (4999, 9999)
    assert Fraction(*a) > Fraction(*b) and nm.device_key(*a) > nm.device_key(*b)
    assert np.float32(a[0]) / np.float32(a[1]) == np.float32(b[0]) / np.float32(b[1]) or np.float32(a[0]) / np.float32(a[1]) < np.float32(b[0]) / np.float32(b[1])


def test_the_strips():
    assert nm.strip_entries_of(300, 300, 128 * 300 * 4) == 128 and nm.stats_of(300, 300, 128 * 300 * 4) == (3, 128, 9)
    assert nm.stats_of(300, 300, 256 * 300 * 4) == (2, 256, 9) and nm.stats_of(300, 300, 1 << 28) == (1, 300, 9)
    assert nm.stats_of(300, 45, 1) == (3, 128, 3) and nm.stats_of(0, 45, 1 << 28) == (0, 0, 0)
    assert nm.pitch_of(45) == 48 and nm.strip_entries_of(1000, 45, 384 * 48 * 4 - 1) == 256
    assert om.tiles_of(300, 300, False) == 9
