"""The case table of search_shapes.py a second time, for groups with DEAD columns: columns retired from the middle of a
resident group, which only the group's valid mask keeps out of a hit list.  Data and pure functions only;
test_search_holes_ledger.py checks them on a CPU, test_gpu_search_holes.py runs them.

- dead_ranges(W): the dead pattern of a group of W columns as [(kind, columns)], every range clipped to [0, W) and dropped
  where nothing of it is left:
    "singles"   columns 0, 1, 2, 127, 128: the first bits of the first 16-byte unit, and a unit boundary
    "unit"      [640, 768): unit 5, whole
    "even"      the even columns of [1152, 1280), unit 9: a slip in the bit or word order of a kernel's mask read
    "group"     [3072, 4096): one whole 128-byte column group, the unit of the screen-to-refine handover
    "boundary"  [8192 s - 8, 8192 s + 8) around every KiB-step boundary s inside the row: where two wave chunks meet
    "step"      rows of 3 KiB-steps and more: the whole KiB-step ch // 2, one wave's chunk
    "tail"      [1024 (W - 1) // 1024, W), the last 128-byte group up to the last column; rows of less than 1 KiB:
                [128 (W - 1) // 128, W), the last unit
- dead_columns(W): their union, sorted.  At most half of W (the ledger checks it).
- hot_columns(W): dead columns that carry, in every row of every planted query of the group's batches (in a count_dense
  group: in every row), a SET bit -- unmasked, such a column is reported for every planted query at every threshold with
  num_match = n: the first and last column of every range (every single column), two in the middle of every range longer
  than 16, every eighth dead column of unit 9.  All other dead columns hold zeros.
- HOLE_CASES: every AND case of search_shapes.CASES; of the count cases those of HOLE_BATCHES, the hash count rotating over
  a test's (batch, shape) rows and not multiplied out (the 32-plane batches c20b, c32r and c32 stay with the unholed table:
  their cost is the query's length and the emit code is the same template); and the cases of ("count_wide", 2) -- three
  KiB-steps, the middle one dead, in front of every count family."""
import re

import numpy as np

import search_shapes as ss
from search_shapes import Case, EE, BOTH, SCREEN, TRUNC, PF

KINDS = ("singles", "unit", "even", "group", "boundary", "step", "tail")


def steps(W):
    """KiB-steps of a row of W columns (its stride is a multiple of 128 bytes)."""
    return (W + 8191) // 8192


def stride_bytes(W):
    return ((W + 7) // 8 + 127) // 128 * 128


def dead_ranges(W):
    ch = steps(W)
    ranges = [("singles", np.array([0, 1, 2, 127, 128])), ("unit", np.arange(640, 768)), ("even", np.arange(1152, 1280, 2)),
              ("group", np.arange(3072, 4096))]
    ranges += [("boundary", np.arange(8192 * s - 8, 8192 * s + 8)) for s in range(1, ch)]
    if ch >= 3:
        ranges.append(("step", np.arange(8192 * (ch // 2), 8192 * (ch // 2 + 1))))
    last = 1024 if stride_bytes(W) >= 1024 else 128
    ranges.append(("tail", np.arange(last * ((W - 1) // last), W)))
    out = []
    for kind, cols in ranges:
        cols = cols[(cols >= 0) & (cols < W)]
        if cols.size:
            out.append((kind, cols))
    return out


def fitting_kinds(W):
    """The kinds of range a row of W columns has room for (a range cut by the row's end still counts)."""
    ch = steps(W)
    return {"singles", "tail"} | {k for k, lo in (("unit", 640), ("even", 1152), ("group", 3072)) if lo < W} | \
        ({"boundary"} if ch >= 2 else set()) | ({"step"} if ch >= 3 else set())


def dead_columns(W):
    return np.unique(np.concatenate([cols for _, cols in dead_ranges(W)]))


def hot_columns(W):
    hot = []
    for kind, cols in dead_ranges(W):
        if kind == "singles":
            hot.append(cols)
            continue
        hot.append(cols[[0, -1]])
        if cols.size > 16:
            hot.append(cols[[cols.size // 3, 2 * cols.size // 3]])
        if kind == "even":
            hot.append(cols[::8])
    return np.unique(np.concatenate(hot))


def real_columns(W, span):
    """bool [span]: what Group.real_columns() must say after the dead columns of a group of W columns are retired."""
    real = np.zeros(span, dtype=bool)
    real[:W] = True
    real[dead_columns(W)] = False
    return real


# ---- the cases -----------------------------------------------------------------------------------------------------------
HOLE_BATCHES = ("c7", "c10", "c14a", "c14b", "c20a", "n7", "n10", "n14")
WIDE = ("count_wide", 2)


def _with_nh(key, nh):
    return (key[0], nh) + tuple(key[2:])


def _shape(c):
    """A count case without its hash count: what the five cases that differ in nh alone share."""
    return (c.test, c.batch, re.sub(r"<(\d+),\d+", r"<\1,*", c.name), _with_nh(c.group, 0), c.t, c.flags, tuple(sorted(c.knobs.items())))


def _rotated(cases):
    """Of cases that come in all five hash counts, one per shape: a test's shapes in table order take the hash counts in
    turn -- hash count nh goes to shape (nh - 1) % m of m, and shapes beyond the fifth take 1 + j % 5 -- so every test runs
    every hash count and every shape once, whatever m is."""
    by_test = {}
    for c in cases:
        shapes = by_test.setdefault(c.test, {})
        shapes.setdefault(_shape(c), {})[c.group[1]] = c
    out = []
    for shapes in by_test.values():
        rows = list(shapes.values())
        m = len(rows)
        picks = [((nh - 1) % m, nh) for nh in ss.NHS] + [(j, 1 + j % 5) for j in range(5, m)]
        out += [rows[j][nh] for j, nh in sorted(picks)]
    return out


def _wide_cases():
    out = []
    for b, p in (("c10", 10), ("c14a", 14)):
        out.append(Case("count_screen", "count_screen_kernel<%d,2>+refine<7>" % p, WIDE, b, 0.8, (EE,), SCREEN))
        out.append(Case("count_walk_trunc", "count_walk_kernel<%d,2,trunc>+refine<7>" % p, WIDE, b, 0.9, (EE,), TRUNC))
        out.append(Case("count_walk_pf", "count_walk_kernel<%d,2,pf%s>" % (p, ",8" if p >= 14 else ""), WIDE, b, 0.9, (0,), PF))
        # (two segments of 64 / 512 k-mers: 7 / 10 planes each)
        out.append(Case("count_segments", "count_kernel<%d,2>+segments->%d" % (ss.planes_for(ss.BATCH_MAX_POS[b] // 2), p), WIDE, b, 0.8, BOTH, dict(force_segs=2)))
        out.append(Case("count_kernel", "count_kernel<%d,2>" % p, WIDE, b, 0.8, BOTH, dict(force_segs=1)))
    return out


WIDE_CASES = _wide_cases()
HOLE_CASES = ([c for c in ss.CASES if c.test.startswith("and")]
              + _rotated([c for c in ss.CASES if not c.test.startswith("and") and c.batch in HOLE_BATCHES]) + WIDE_CASES)

# The two groups the other search forms (presence, top-k, scores) run on, with the batch and threshold of each.
OTHER_FORMS = ((("and", 5), "and", 1.0), (("count", 2), "c10", 0.8))
