"""The ledger of tests/search_holes.py (no GPU): the dead pattern is what its docstring says on every group the holed cases
use, and the holed selection of search_shapes.CASES still launches every gather-kernel family and, within each family,
every value of every template argument that indexes the row, every hash count and every counter width its batches can
give.  A family or a value lost from HOLE_CASES fails here, naming it."""
import numpy as np

import search_holes as sh
import search_shapes as ss

# The template integers of launched()'s keys, by family: "nh" the hash count, "p" counter planes, "c" a constant of the
# name; everything else indexes the row (vectors per lane, KiB-steps, units or unroll, queries per wave, segments or not,
# truncated or prefetching, the refine units' width).
ARGS = {
    "and_narrow_kernel": ("G", "U"), "and_screen_kernel": ("VEC", "c"), "and_refine_kernel": ("U",), "and_refine_emit_kernel": (),
    "band_bucket_kernel": (), "and_band_walk_kernel": ("CH", "c"), "and_band_finish_kernel": ("CH",), "and_walk_kernel": ("CH", "U"),
    "and_kernel": ("VEC", "segments"), "and_combine_kernel": (),
    "count_screen_kernel": ("p", "nh"), "count_refine_kernel": ("nh", "UP"), "count_refine_emit_kernel": ("p", "UP"),
    "count_walk_kernel": ("p", "nh", "trunc"), "count_kernel": ("p", "nh", "segments"), "count_combine_kernel": ("p",),
    "count_narrow_kernel": ("p", "nh", "G"),
}


def values(cases):
    """{family: [set of values per template argument]} over everything the cases launch."""
    out = {}
    for c in cases:
        for fam, a in ss.launched(c.name):
            got = out.setdefault(fam, [set() for _ in a])
            for s, v in zip(got, a):
                s.add(v)
    return out


def group_keys():
    return list(dict.fromkeys(c.group for c in sh.HOLE_CASES))


def test_dead_pattern_on_every_group():
    keys = group_keys()
    assert {k[0] for k in keys} == {"and", "and_wide", "and_narrow", "count", "count_narrow", "count_wide"}
    for key in keys:
        W = ss.group_shape(key)[0]
        nb = (W + 7) // 8
        dead, hot = sh.dead_columns(W), sh.hot_columns(W)
        assert np.array_equal(dead, np.unique(dead)) and dead[0] >= 0 and dead[-1] == W - 1, key
        assert 2 * dead.size <= W, (key, dead.size, W)
        assert np.isin(hot, dead).all() and 0 < hot.size < dead.size, key
        kinds = [k for k, _ in sh.dead_ranges(W)]
        assert set(kinds) == sh.fitting_kinds(W) and set(kinds) <= set(sh.KINDS), (key, kinds)
        assert kinds.count("boundary") == sh.steps(W) - 1, key
        # the first and last column of every range are hot, and dead columns that are not hot exist inside every longer range
        for kind, cols in sh.dead_ranges(W):
            assert np.isin(cols[[0, -1]], hot).all(), (key, kind)
            assert kind == "singles" or cols.size <= 2 or not np.isin(cols, hot).all(), (key, kind)
        # the bytes every group plants columns in: one loses all its columns, one keeps a live column beside a dead one
        isdead = np.zeros(8 * nb, dtype=bool)
        isdead[dead] = True
        isdead[W:] = True                                  # (pad bits are no columns)
        spots = ss.planted_edges(nb)[:7]
        per = isdead.reshape(nb, 8)[spots]
        assert per.all(axis=1).any(), (key, "no planted byte is wholly dead")
        assert (per.any(axis=1) & ~per.all(axis=1)).any(), (key, "no planted byte is partly alive")
    # the pattern itself, pinned on the narrowest and on a wide row
    assert sh.dead_columns(997).tolist() == [0, 1, 2, 127, 128] + list(range(640, 768)) + list(range(896, 997))
    W = 8192 * 3 - 93
    want = set([0, 1, 2, 127, 128]) | set(range(640, 768)) | set(range(1152, 1280, 2)) | set(range(3072, 4096)) | set(range(8184, 16392)) | set(range(23552, W))
    assert set(sh.dead_columns(W).tolist()) == want
    assert sh.dead_columns(1997)[-77:].tolist() == list(range(1920, 1997)) and 1919 not in sh.dead_columns(1997)      # rows under 1 KiB: the last unit
    assert sh.real_columns(997, 1000).sum() == 997 - 234 and not sh.real_columns(997, 1000)[997:].any()


def test_hole_cases_are_a_selection():
    names = set(ss.printable_names())
    for i, c in enumerate(sh.HOLE_CASES):
        assert c in ss.CASES or c.group == sh.WIDE, c
        assert c.name in names or c.group == sh.WIDE, c
        assert c.batch in sh.HOLE_BATCHES or c.test.startswith("and"), c
        assert ss.launched(c.name), c
        assert c not in sh.HOLE_CASES[:i], c
    assert [c for c in ss.CASES if c.test.startswith("and")] == [c for c in sh.HOLE_CASES if c.test.startswith("and")]
    # the wide count group: one case of each count form per batch, the names the same template arguments but the planes
    assert ss.group_shape(sh.WIDE) == (8192 * 3 - 93, 2, 14)
    for b in ("c10", "c14a"):
        assert sorted(c.test for c in sh.WIDE_CASES if c.batch == b) == ["count_kernel", "count_screen", "count_segments", "count_walk_pf", "count_walk_trunc"]
    for c in sh.WIDE_CASES:
        twin = [d for d in ss.CASES if d.test == c.test and d.batch == c.batch and d.group == ("count", 2) and d.knobs == c.knobs]
        assert len(twin) == 1 and {(f, a[1:]) for f, a in ss.launched(c.name)} == {(f, a[1:]) for f, a in ss.launched(twin[0].name)}, c
    for g, b, t in sh.OTHER_FORMS:
        assert any(c.group == g and c.batch == b and c.t == t for c in sh.HOLE_CASES), (g, b, t)


def test_hole_cases_launch_every_family_and_argument():
    got = values(sh.HOLE_CASES)
    assert set(got) == set(ss.GATHER_FAMILIES), set(ss.GATHER_FAMILIES) ^ set(got)
    assert set(ARGS) == set(ss.GATHER_FAMILIES)
    # what the unholed table reaches with the batches the holed one may use: the most a selection can reach
    pool = values([c for c in ss.CASES if c.test.startswith("and") or c.batch in sh.HOLE_BATCHES])
    for fam, kinds in ARGS.items():
        assert len(kinds) == len(got[fam]), fam
        for kind, have, most in zip(kinds, got[fam], pool[fam]):
            if kind == "nh":
                assert have == set(ss.NHS), (fam, "hash counts", sorted(set(ss.NHS) - have))
            elif kind == "p":
                assert have >= most and most & {7, 10, 14, 20} == have & {7, 10, 14, 20}, (fam, "planes", sorted(most - have))
                assert have & {7, 10, 14, 20}, fam
            else:
                assert have == most, (fam, kind, sorted(most - have))
    # and the values themselves, where the engine has more than one
    assert got["and_walk_kernel"][0] == set(range(1, 17)) and got["and_walk_kernel"][1] == {4, 8}
    assert got["and_band_walk_kernel"][0] == got["and_band_finish_kernel"][0] == set(range(3, 17))
    assert got["and_kernel"] == [{1, 2, 4}, {0, 1}] and got["and_screen_kernel"][0] == {1, 2} and got["and_refine_kernel"] == [{8, 16}]
    assert got["and_narrow_kernel"] == [{8, 4, 2}, {16, 8}]
    assert got["count_kernel"][2] == {0, 1} and got["count_walk_kernel"][2] == {0, 1} and got["count_narrow_kernel"][2] == {4, 2}
    assert got["count_refine_kernel"][1] == {7, 14} and got["count_refine_emit_kernel"][1] == {7, 14}
    assert got["count_screen_kernel"][0] == {7, 10, 14} and got["count_walk_kernel"][0] == {7, 10, 14, 20}
    assert got["count_kernel"][0] >= {7, 10, 14} and got["count_combine_kernel"][0] == {7, 10, 14} and got["count_narrow_kernel"][0] == {7, 10, 14}
    # every test of the table has cases, and the wide group adds a case to each count form it can run
    assert {c.test for c in sh.HOLE_CASES} == {c.test for c in ss.CASES}
