"""The gather stage of kwage_search (engine.hip, launch_search_stage) stated as data: which kernel instantiations a reported
`search_kernel` name launches, and the table of cases that together launch every one of them.

- GATHER_FAMILIES: the gather-stage kernel families (not the k-mer stage, the loaders or the read probe).
- launched(name): {(family, template ints)} -- every kernel the search that reports `name` launches.
- printable_names(): every name engine.hip can report, by format string (FORMATS: the format strings themselves).
- UNREACHABLE: instantiations the dispatch compiles but can never launch, each with the reason.
- CASES: what test_gpu_search_shapes.py runs -- group, batch, threshold, flags, knobs -- and the exact name each case must
  report.  test_search_shapes_ledger.py checks on CPU that the cases launch every instantiation of the gfx950 assembly.

Group keys (GROUP_SHAPES; built by test_gpu_search_shapes.py; W columns, 2^L rows, NH hashes; group_fill: the share of set
bits the common columns are drawn with):
  ("and", CH)          W = 8192 CH - 93: rows of CH KiB-steps, NH = 1 + (CH - 1) % 5, L = 12
  ("and_wide",)        W = 8192 * 17 - 93: rows above 16 KiB, NH = 2, L = 12
  ("and_narrow", G)    W = 997 / 1997 / 3997 for G = 8 / 4 / 2, NH = 3, L = 12
  ("count", NH)        W = 8099 (one KiB-step, one column tile), L = 17
  ("count_narrow", NH, G)  W = 1997 / 3997 for G = 4 / 2, L = 14
  ("count_dense", NH)  W = 997, L = 12, columns of all ones: counts above 2^20
  ("count_wide", NH)   W = 8192 * 3 - 93: three KiB-steps in front of the count kernels, L = 14 (search_holes.py's cases only)
Batch keys: BATCH_MAX_POS gives each batch's longest query in k-mer positions (k = 31); "and_many" and "and_wide" are sized
from the device's CU count (CU_SIZED, batch_size).  batch_seqs(key, ncu) makes a batch's sequences -- the GPU test searches
them, test_search_plan.py feeds their lengths to the host-side plan (kwage_amd/csrc/search_plan.hpp).  The count batches c10, c14a and c20a sit at the lower edge of their counter width
(128, 1024, 16384 positions): a column holding every k-mer of the longest query needs the width's top plane."""
import re
from collections import namedtuple

import numpy as np

from topk_reference import rand_seq

GATHER_FAMILIES = frozenset({
    "and_kernel", "and_combine_kernel", "and_narrow_kernel", "and_walk_kernel", "and_screen_kernel", "and_refine_kernel",
    "and_refine_emit_kernel", "band_bucket_kernel", "and_band_walk_kernel", "and_band_finish_kernel",
    "count_kernel", "count_combine_kernel", "count_narrow_kernel", "count_walk_kernel", "count_screen_kernel",
    "count_refine_kernel", "count_refine_emit_kernel",
})

# Compiled, never launched.  Each entry: the instantiation and why no input reaches it.
UNREACHABLE = {
    ("and_narrow_kernel", (16, 8)): "G = 16 needs rows of <= 4 16-byte units, but a group's row stride is a multiple of 128 bytes (8 units)",
    ("and_narrow_kernel", (16, 16)): "as <16,8>",
    ("count_refine_emit_kernel", (32, 7)): "7-plane units need every query's remainder <= 15360 k-mers, but a truncated query of "
                                           "more than 2^20 positions keeps at least 15 % of them, and an untruncated one keeps the batch "
                                           "from truncating at all",
}

PLANES = (7, 10, 14, 20, 32)
NHS = (1, 2, 3, 4, 5)


def planes_for(max_count):
    """search_plan.hpp planes_for: the narrowest counter width whose bits hold max_count."""
    bits = 1
    while bits < 32 and (max_count >> bits) != 0:
        bits += 1
    return 7 if bits <= 7 else 10 if bits <= 10 else 14 if bits <= 14 else 20 if bits <= 20 else 32


_I = r"(\d+)"
_PATTERNS = [
    (r"and_narrow_kernel<%s,%s>" % (_I, _I), lambda g, u: {("and_narrow_kernel", (g, u))}),
    (r"and_screen_kernel<%s,8>\+refine<%s>" % (_I, _I),
     lambda v, u: {("and_screen_kernel", (v, 8)), ("and_refine_kernel", (u,)), ("and_refine_emit_kernel", ())}),
    (r"and_band_walk_kernel<%s,4>" % _I,
     lambda ch: {("band_bucket_kernel", ()), ("and_band_walk_kernel", (ch, 4)), ("and_band_finish_kernel", (ch,))}),
    (r"and_walk_kernel<%s,%s>" % (_I, _I), lambda ch, u: {("and_walk_kernel", (ch, u))}),
    (r"and_kernel<%s,8,nt>" % _I, lambda v: {("and_kernel", (v, 0))}),
    (r"and_kernel<%s,8,nt>\+segments" % _I, lambda v: {("and_kernel", (v, 1)), ("and_combine_kernel", ())}),
    (r"count_screen_kernel<%s,%s>\+refine<%s>" % (_I, _I, _I),
     lambda p, nh, up: {("count_screen_kernel", (p, nh)), ("count_refine_kernel", (nh, up)), ("count_refine_emit_kernel", (p, up))}),
    (r"count_walk_kernel<%s,%s,trunc>\+refine<%s>" % (_I, _I, _I),
     lambda p, nh, up: {("count_walk_kernel", (p, nh, 1)), ("count_refine_kernel", (nh, up)), ("count_refine_emit_kernel", (p, up))}),
    (r"count_walk_kernel<%s,%s,pf>" % (_I, _I), lambda p, nh: {("count_walk_kernel", (p, nh, 0))} if p < 14 else None),
    (r"count_walk_kernel<%s,%s,pf,8>" % (_I, _I), lambda p, nh: {("count_walk_kernel", (p, nh, 0))} if p >= 14 else None),
    (r"count_kernel<%s,%s>\+segments->%s" % (_I, _I, _I),
     lambda sp, nh, p: {("count_kernel", (sp, nh, 1)), ("count_combine_kernel", (p,))} if sp <= p else None),
    (r"count_kernel<%s,%s>" % (_I, _I), lambda p, nh: {("count_kernel", (p, nh, 0))}),
    # (the one name that prints the hash count unclamped: the header allows 1..5 only, clamped here like the others)
    (r"count_narrow_kernel<%s,%s,%s,8>" % (_I, _I, _I), lambda p, nh, g: {("count_narrow_kernel", (p, min(nh, 5), g))}),
]


def launched(name):
    """-> set of (family, template ints) that the search reporting `name` launches (ValueError: not a name engine.hip prints)."""
    for pat, fn in _PATTERNS:
        m = re.fullmatch(pat, name)
        if m:
            out = fn(*(int(x) for x in m.groups()))
            if out is None:
                break
            return out
    raise ValueError("not a search_kernel name of engine.hip: %r" % name)


# The format strings of search_plan.hpp's format_search_name and the arguments each can be given.
FORMATS = {
    "and_narrow_kernel<%u,%d>": ["and_narrow_kernel<%d,%d>" % (g, u) for g in (8, 4, 2) for u in (16, 8)],
    "and_screen_kernel<%d,8>+refine<%d>": ["and_screen_kernel<%d,8>+refine<%d>" % (v, u) for v in (1, 2) for u in (8, 16)],
    "and_band_walk_kernel<%u,4>": ["and_band_walk_kernel<%d,4>" % ch for ch in range(3, 17)],
    "and_walk_kernel<%u,%d>": ["and_walk_kernel<%d,%d>" % (ch, 8 if ch <= 2 else 4) for ch in range(1, 17)],
    "and_kernel<%d,8,nt>%s": ["and_kernel<%d,8,nt>%s" % (v, s) for v in (1, 2, 4) for s in ("", "+segments")],
    "count_screen_kernel<%u,%u>+refine<%d>": ["count_screen_kernel<%d,%d>+refine<%d>" % (p, nh, up)
                                              for p in (7, 10, 14) for nh in NHS for up in ((7, 14) if p == 14 else (7,))],
    "count_walk_kernel<%u,%u,trunc>+refine<%d>": ["count_walk_kernel<%d,%d,trunc>+refine<%d>" % (p, nh, up)
                                                  for p in (10, 14, 20, 32) for nh in NHS
                                                  for up in ((7,) if p < 14 else (14,) if p == 32 else (7, 14))],
    "count_walk_kernel<%u,%u,pf%s>": ["count_walk_kernel<%d,%d,pf%s>" % (p, nh, ",8" if p >= 14 else "") for p in PLANES for nh in NHS],
    "count_narrow_kernel<%u,%u,%d,%d>": ["count_narrow_kernel<%d,%d,%d,8>" % (p, nh, g) for p in (7, 10, 14) for nh in NHS for g in (4, 2)],
    "count_kernel<%u,%u>+segments->%u": ["count_kernel<%d,%d>+segments->%d" % (sp, nh, p) for p in PLANES for sp in PLANES if sp <= p for nh in NHS],
    "count_kernel<%u,%u>": ["count_kernel<%d,%d>" % (p, nh) for p in PLANES for nh in NHS],
}


def printable_names():
    return [n for names in FORMATS.values() for n in names]


# ---- the case table ------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "test name group batch t flags knobs")
EE = 1          # KWAGE_SEARCH_EARLY_EXIT
BOTH = (0, EE)

BATCH_MAX_POS = {"and": 370, "and_short": 100, "and_many": 100, "and_wide": 100,
                 "c7": 127, "c10": 128, "c14a": 1024, "c14b": 12000, "c20a": 16384, "c20b": 40000,
                 "c32r": (1 << 21) + 100, "c32": (1 << 21) + 100, "n7": 127, "n10": 1023, "n14": 3000}
CU_SIZED = ("and_many", "and_wide")       # query counts from the device's CU count (batch_size)
K = 31

GROUP_SHAPES = {"and": lambda ch: (8192 * ch - 93, 1 + (ch - 1) % 5, 12), "and_wide": lambda: (8192 * 17 - 93, 2, 12),
                "and_narrow": lambda g: ({8: 997, 4: 1997, 2: 3997}[g], 3, 12), "count": lambda nh: (8099, nh, 17),
                "count_narrow": lambda nh, g: ({4: 1997, 2: 3997}[g], nh, 14), "count_dense": lambda nh: (997, nh, 12),
                "count_wide": lambda nh: (8192 * 3 - 93, nh, 14)}


def group_shape(key):
    """-> (W columns, NH hashes, L: 2^L rows) of the group `key`."""
    return GROUP_SHAPES[key[0]](*key[1:])


def group_fill(key):
    """The probability the bits of the group's common columns are set with."""
    return 0.25 if key[0].startswith("and") else (0.02, 0.14, 0.27, 0.38, 0.46)[group_shape(key)[1] - 1]


def planted_edges(nb):
    """The bytes of a row of nb bytes that hold a group's planted columns first: the row's ends, the first unit boundary, the
    first 128-byte boundary, the middle and both sides of every KiB-step boundary."""
    edges = [0, 15, 16, 127, 128, nb // 2, nb - 1] + [j for s in range(1024, nb, 1024) for j in (s - 1, s)]
    return list(dict.fromkeys(e for e in edges if 0 <= e < nb))


def batch_size(ncu, key):
    return {"and_many": 16 * ncu * 8, "and_wide": (8 * ncu + 4) // 5 + 8}[key]


def _period_query(rng, npos, period):
    unit = rand_seq(rng, period)
    n = npos + K - 1
    return (unit * (n // period + 1))[:n]


def batch_seqs(key, ncu):
    """-> (seqs, plant): the sequences of batch `key` on a device of ncu CUs, and the indices of those whose rows the groups
    plant columns from.  A function of (key, ncu) only."""
    mp = BATCH_MAX_POS[key]
    rng = np.random.default_rng(mp + (1 if key == "c32r" else 0))       # (batches of one length share their pool)
    longest = mp + K - 1
    if key == "c32":
        seqs = [rand_seq(rng, longest), rand_seq(rng, 500), "ACGT" * 10]
        plant = [0, 1]
    elif key == "c32r":
        seqs = [_period_query(rng, mp, 4001), rand_seq(rng, 3000), rand_seq(rng, 800)]
        plant = [0, 1, 2]
    elif key.startswith("and") or key.startswith("n"):
        pool = [rand_seq(rng, longest)] + [rand_seq(rng, int(rng.integers(K + 4, longest + 1))) for _ in range(28)]
        pool += [rand_seq(rng, K), "", "ACGTN" * 4, pool[3][:40] + "N" + pool[3][41:], pool[5]]   # one k-mer, none, none, an N, repeated
        n = batch_size(ncu, key) if key in CU_SIZED else {"and": len(pool), "and_short": 2000, "n7": 96, "n10": 96, "n14": 96}[key]
        seqs = [pool[i % len(pool)] for i in range(n)]
        plant = list(range(29))
    else:           # the count batches: a few long queries, shorter ones and the edge queries
        seqs = [rand_seq(rng, longest)]
        for f in (0.9, 0.6, 0.3):
            seqs.append(rand_seq(rng, max(int(longest * f), K + 70)))
        base = seqs[1]
        mutated = list(base)
        for p in range(11, len(mutated), 97):            # substitutions: counts between the threshold and n
            mutated[p] = "ACGT"[("ACGT".index(mutated[p]) + 1) % 4]
        seqs += ["".join(mutated), rand_seq(rng, 100), rand_seq(rng, K), "", "N" * 60, seqs[2]]
        plant = [0, 1, 2, 3, 5]
    assert max(max(len(s) - K + 1, 0) for s in seqs) == mp, (key, mp)
    return seqs, plant

WALK = dict(walk=4, walk_min_rows=1, walk_min_kib=1, walk_bands=0)
BAND = dict(walk=4, walk_min_rows=1, walk_min_kib=1, walk_bands=3, walk_bands_min_gib=0)
SCREEN = dict(count_screen_min_tiles=1)
TRUNC = dict(count_walk_min_rows=1, count_screen_min_tiles=1 << 30)
PF = dict(count_walk_min_rows=1)


def _and_cases():
    out = []
    for G in (8, 4, 2):          # (U = 16 below 16 x CUs x G queries: "and_short"; U = 8 at "and_many")
        out.append(Case("and_narrow", "and_narrow_kernel<%d,16>" % G, ("and_narrow", G), "and_short", 1.0, (0,), {}))
        out.append(Case("and_narrow", "and_narrow_kernel<%d,8>" % G, ("and_narrow", G), "and_many", 1.0, (0,), {}))
    for ch, v in ((2, 1), (5, 2)):
        for u in (8, 16):
            out.append(Case("and_screen", "and_screen_kernel<%d,8>+refine<%d>" % (v, u), ("and", ch), "and", 1.0, (EE,), dict(refine_unroll=u)))
    for ch in range(1, 17):
        out.append(Case("and_walk", "and_walk_kernel<%d,%d>" % (ch, 8 if ch <= 2 else 4), ("and", ch), "and", 1.0, (0,), WALK))
        out.append(Case("and_band_walk", "and_walk_kernel<%d,8>" % ch if ch <= 2 else "and_band_walk_kernel<%d,4>" % ch,
                        ("and", ch), "and", 1.0, (0,), BAND))
    for v in (1, 2, 4):
        for segs in (1, 3):
            out.append(Case("and_kernel", "and_kernel<%d,8,nt>%s" % (v, "+segments" if segs > 1 else ""), ("and", 4), "and", 1.0, BOTH,
                            dict(walk=0, and_vec=v, force_segs=segs)))
    out.append(Case("and_kernel", "and_kernel<4,8,nt>", ("and_wide",), "and_wide", 1.0, (0,), {}))     # the natural wide shape
    return out


def _count_cases():
    out = []
    for nh in NHS:
        g = ("count", nh)
        for b, p, up in (("c7", 7, 7), ("c10", 10, 7), ("c14a", 14, 7), ("c14b", 14, 14)):
            out.append(Case("count_screen", "count_screen_kernel<%d,%d>+refine<%d>" % (p, nh, up), g, b, 0.8, (EE,), SCREEN))
        for b, p, up in (("c10", 10, 7), ("c14a", 14, 7), ("c20a", 20, 7), ("c20b", 20, 14), ("c32r", 32, 14)):
            out.append(Case("count_walk_trunc", "count_walk_kernel<%d,%d,trunc>+refine<%d>" % (p, nh, up), g, b, 0.9, (EE,), TRUNC))
        for b in ("c7", "c10", "c14a", "c20b", "c32r"):
            p = planes_for(BATCH_MAX_POS[b])
            out.append(Case("count_walk_pf", "count_walk_kernel<%d,%d,pf%s>" % (p, nh, ",8" if p >= 14 else ""), g, b, 0.9, (0,), PF))
        for b in ("c7", "c10", "c14a", "c20b"):
            out.append(Case("count_kernel", "count_kernel<%d,%d>" % (planes_for(BATCH_MAX_POS[b]), nh), g, b, 0.8, BOTH, dict(force_segs=1)))
        # segments: SP = the planes of one segment's k-mers, P = the query's
        for b, segs in (("c7", 2), ("c10", 2), ("c14a", 2), ("c14a", 100), ("c20b", 2), ("c20b", 7)):
            mp = BATCH_MAX_POS[b]
            sp = planes_for(-(-mp // segs))          # (engine.hip choose_segments: ceil(max / segs) k-mers per segment)
            out.append(Case("count_segments", "count_kernel<%d,%d>+segments->%d" % (sp, nh, planes_for(mp)), g, b, 0.8, BOTH, dict(force_segs=segs)))
        d = ("count_dense", nh)
        out.append(Case("count_kernel", "count_kernel<32,%d>" % nh, d, "c32", 0.9, (0,), dict(force_segs=1)))
        out.append(Case("count_walk_pf", "count_walk_kernel<32,%d,pf,8>" % nh, d, "c32", 0.9, (0,), PF))
        for segs in (2, 3):
            mp = BATCH_MAX_POS["c32"]
            sp = planes_for(-(-mp // segs))          # (engine.hip choose_segments: ceil(max / segs) k-mers per segment)
            out.append(Case("count_segments", "count_kernel<%d,%d>+segments->32" % (sp, nh), d, "c32", 0.9, (0,), dict(force_segs=segs)))
        for G in (4, 2):
            for b in ("n7", "n10", "n14"):
                out.append(Case("count_narrow", "count_narrow_kernel<%d,%d,%d,8>" % (planes_for(BATCH_MAX_POS[b]), nh, G),
                                ("count_narrow", nh, G), b, 0.8, BOTH, dict(force_segs=1)))
    return out


CASES = _and_cases() + _count_cases()
