"""The table of cases the compaction's tests share (tests/test_compact_cases.py checks the table itself without a device,
tests/test_gpu_compact.py runs it through the C ABI), and the numpy reference: the matrix after the call is
np.packbits(image[:, valid], axis=1, bitorder="little"), new_column the rank among the valid columns.

A case is built from file-like blocks (Group.add_columns: each starts on a 16-byte boundary of the row), then live inserts
(the first on a 16-byte boundary, the next ones at bit granularity), then a retired set.  `grow` widens the case's main
block so that the number of survivors m lands on a wanted residue: every case runs with m % 128 == 0 and m % 128 == 1
(which is also m % 8 != 0) where it allows it."""
from collections import namedtuple

import numpy as np

UNIT = 128                  # columns of a 16-byte unit
SEGMENT = 256               # units of a segment of a wide row: the kernel's workgroup size (compact_kernels.hpp)

Case = namedtuple("Case", "name blocks inserts retired edge grow after")
# blocks / inserts: column counts; retired(columns) -> the retired ones, `columns` the ascending list of real columns;
# grow: the index of the block that residues may widen (None: the case's shape is fixed); after: filters inserted after
# the compaction


def _a(cols): return [cols[0]]
def _b(cols): return cols[:33005]
def _c(cols): return [cols[40000]]
def _d(cols): return cols[1000:1512:2]
def _e(cols): return cols[128:256] + cols[4096:5120]
def _f(cols): return [cols[i] for i in (31, 32, 127, 128, 129)]
def _g(cols): return cols[-200:]
def _h(cols): return list(cols)
def _i(cols): return []
def _j(cols): return [cols[-6]]             # the third filter of the first insert


CASES = [
    Case("a", [70000], [], _a, "a shift of one bit over several segments: the barrier's case", 0, 0),
    Case("b", [70000], [], _b, "sources more than a whole segment ahead", 0, 0),
    Case("c", [70000], [], _c, "an untouched identity prefix", 0, 0),
    Case("d", [6000], [], _d, "runs of one", 0, 0),
    Case("e", [6000], [], _e, "whole units retired", 0, 0),
    Case("f", [6000], [], _f, "holes across 32-bit and 128-bit boundaries", 0, 0),
    Case("g", [6000], [], _g, "nothing moves, the span shrinks", 0, 0),
    Case("h", [6000], [], _h, "m = 0", None, 0),
    Case("i", [70, 1, 300], [], _i, "only alignment pads; a 128-byte stride, several rows per workgroup", None, 0),
    Case("j", [300, 900], [5, 3], _j, "inserts after the compaction land at columns m .. m + 3", 1, 4),
]
RESIDUES = (0, 1)


def sized(case, residue):
    """The case with its main block widened (by less than a unit) until m % 128 == residue; a fixed case as it is."""
    if case.grow is None:
        return case
    for extra in range(UNIT):
        blocks = list(case.blocks)
        blocks[case.grow] += extra
        c = case._replace(blocks=blocks)
        if layout(c).m % UNIT == residue:
            return c
    raise AssertionError(case.name)


Layout = namedtuple("Layout", "span tail columns retired valid m new_column capacity")


def layout(case):
    """Where the case's columns lie before the compaction and what the call has to make of them."""
    next_byte, columns = 0, []
    for n in case.blocks:
        start = (next_byte + 15) // 16 * 16
        columns.extend(range(8 * start, 8 * start + n))
        next_byte = start + (n + 7) // 8
    tail = None
    for n in case.inserts:
        first = (next_byte + 15) // 16 * 16 * 8 if tail is None else tail
        columns.extend(range(first, first + n))
        tail = first + n
        next_byte = (tail + 7) // 8
    span = 8 * next_byte
    retired = sorted(case.retired(columns))
    valid = np.zeros(span, dtype=bool)
    valid[columns] = True
    valid[retired] = False
    new_column = np.where(valid, np.cumsum(valid) - 1, -1).astype(np.int64)
    # (a group's stride is its capacity rounded up to 128 bytes; the tests create the group with this capacity)
    capacity = max(span, 8) + 64
    return Layout(span, tail, columns, retired, valid, int(valid.sum()), new_column, capacity)


def image(case, nrows, seed=0):
    """bool [nrows, span]: random bits on the case's real columns (the retired ones included: retire clears them), pads 0."""
    lay = layout(case)
    rng = np.random.default_rng(seed + 1000 * len(case.name) + lay.span)
    img = np.zeros((nrows, lay.span), dtype=bool)
    img[:, lay.columns] = rng.random((nrows, len(lay.columns))) < 0.4
    return img


def reference(img, valid):
    """The rows after the compaction: uint8 [nrows, ceil(m / 8)]."""
    return np.packbits(img[:, valid], axis=1, bitorder="little")


def plan(lay):
    """What kwage_compact_stats must report for the layout: the runs, the first unit rewritten and how many."""
    v = lay.valid
    idx = np.flatnonzero(v)
    runs = int(1 + np.count_nonzero(np.diff(idx) != 1)) if idx.size else 0
    invalid = np.flatnonzero(~v)
    p = int(invalid[0]) if invalid.size else lay.span
    tail = lay.span if lay.tail is None else lay.tail
    if p >= tail or lay.m == 0:
        first_unit, units = 0, 0
    else:
        first_unit = p // UNIT
        units = (lay.span + UNIT - 1) // UNIT - first_unit
    return {"span_before": lay.span, "span_after": 8 * ((lay.m + 7) // 8), "columns": lay.m, "runs": runs,
            "first_unit": first_unit, "units": units}


def schedule(units, threads=SEGMENT):
    """(threads that share a row, rows per workgroup, segments) for a row of `units` units to rewrite."""
    lanes = 8
    while lanes < threads and lanes < units:
        lanes *= 2
    return lanes, threads // lanes, (units + lanes - 1) // lanes
