"""The contract of the nearest-neighbour lists (include/kwage_amd.h: kwage_group_column_neighbors) in plain Python: the
cells are overlap_model.overlaps', the bits column sums under the valid mask, the keys Python integers or
fractions.Fraction, the order a sort by (-key, index).  None of the planners, never the code under test.  And what the
header says of the strips, for the stats the device tests compare."""
from fractions import Fraction

import numpy as np

import overlap_model as om

SHARED, JACCARD = "shared", "jaccard"
FILLER = (0xFFFFFFFF, 0, 0, 0)
K_MAX = 1024


def key_of(metric, shared, bits_a, bits_b):
    """The key of a pair as an exact number: larger is better."""
    if metric == SHARED:
        return int(shared)
    union = int(bits_a) + int(bits_b) - int(shared)
    return Fraction(int(shared), union) if union else Fraction(0)


def device_key(s, u):
    """The header's scalar key of the fraction s / u: floor(s 2^64 / u) by two 64-bit divisions, all ones for s == u, 0
    for an empty union."""
    if u == 0:
        return 0
    if s == u:
        return (1 << 64) - 1
    q1, r1 = divmod(s << 32, u)
    assert q1 < 1 << 32 and r1 << 32 < 1 << 64
    return (q1 << 32) | ((r1 << 32) // u)


def select(cells, cols_a, live_a, bits_a, cols_b, live_b, bits_b, k, metric, min_shared=0, skip_same=False):
    """(records uint32 [n_a, k, 4], counts uint32 [n_a]) from the cells [n_a, n_b]: cols_x the column every entry names,
    live_x / bits_x per COLUMN of the group; skip_same: a candidate naming the entry's own column is not eligible."""
    n_a, n_b = cells.shape
    records = np.zeros((n_a, k, 4), dtype=np.uint32)
    records[:, :] = FILLER
    counts = np.zeros(n_a, dtype=np.uint32)
    for i in range(n_a):
        ca = int(cols_a[i])
        if not live_a[ca]:
            continue
        found = []
        for j in range(n_b):
            cb = int(cols_b[j])
            s = int(cells[i, j])
            if live_b[cb] and s >= min_shared and not (skip_same and ca == cb):
                found.append((-key_of(metric, s, bits_a[ca], bits_b[cb]), j, s, int(bits_a[ca]), int(bits_b[cb])))
        found.sort(key=lambda t: t[:2])
        counts[i] = min(k, len(found))
        for r, (_, j, s, ba, bb) in enumerate(found[:k]):
            records[i, r] = (j, s, ba, bb)
    return records, counts


def bits_of(bits, valid):
    """Set bits per column: the column sums of bool [rows, >= span] under the valid mask [span]."""
    span = len(valid)
    return (bits[:, :span] & valid[None, :]).sum(axis=0).astype(np.int64)


def of_models(ma, cols_a, mb, cols_b, k, metric, min_shared=0, skip_self=False, same_group=None):
    """select() of two tests/group_model.py GroupModels (mb None: a's list is also the candidate list).  same_group:
    whether b is a's own group (default: mb is None or mb is ma)."""
    if mb is None:
        mb, cols_b = ma, cols_a
        same_group = True
    elif same_group is None:
        same_group = mb is ma
    cells = om.overlaps(ma.bits, ma.real, cols_a, mb.bits, mb.real, cols_b)
    la = np.arange(ma.span) if cols_a is None else np.asarray(cols_a, dtype=np.int64)
    lb = np.arange(mb.span) if cols_b is None else np.asarray(cols_b, dtype=np.int64)
    return select(cells, la, ma.real, bits_of(ma.bits, ma.real), lb, mb.real, bits_of(mb.bits, mb.real), k, metric, min_shared,
                  skip_self and same_group)


def select_loop(bits_a, valid_a, cols_a, bits_b, valid_b, cols_b, k, metric, min_shared=0, skip_same=False):
    """The same lists bit by bit, with no matrix product and no sort: the r-th record is the best of those not yet taken."""
    rows = bits_a.shape[0]
    records, counts = [], []
    for ca in cols_a:
        found = []
        ba = sum(1 for r in range(rows) if bits_a[r, ca]) if valid_a[ca] else 0
        for j, cb in enumerate(cols_b):
            if not (valid_a[ca] and valid_b[cb]) or (skip_same and ca == cb):
                continue
            bb = sum(1 for r in range(rows) if bits_b[r, cb])
            s = sum(1 for r in range(rows) if bits_a[r, ca] and bits_b[r, cb])
            if s >= min_shared:
                found.append((j, s, ba, bb))
        mine = []
        while found and len(mine) < k:
            best = found[0]
            for f in found[1:]:
                # better: a larger fraction s / u by cross-multiplication (or more shared bits); found is in index order
                if metric == SHARED:
                    better = f[1] > best[1]
                else:
                    uf, ub = f[2] + f[3] - f[1], best[2] + best[3] - best[1]
                    better = (f[1] if uf else 0) * (ub or 1) > (best[1] if ub else 0) * (uf or 1)
                if better:
                    best = f
            found.remove(best)
            mine.append(best)
        counts.append(len(mine))
        records.append(mine + [FILLER] * (k - len(mine)))
    return np.array(records, dtype=np.uint32).reshape(len(cols_a), k, 4), np.array(counts, dtype=np.uint32)


# ---- the strips, as the header states them ----

def pitch_of(n_b):
    return (n_b + 3) // 4 * 4


def strip_entries_of(n_a, n_b, strip_bytes):
    """Entries of a full strip: the largest multiple of 128 whose cells (rows of the candidates rounded up to a multiple
    of 4) fit strip_bytes, at least 128, at most n_a."""
    e = strip_bytes // (max(pitch_of(n_b), 4) * 4) // 128 * 128
    return min(max(e, 128), n_a)


def stats_of(n_a, n_b, strip_bytes):
    """(strips, strip_entries, tiles) of a call."""
    if n_a == 0:
        return 0, 0, 0
    e = strip_entries_of(n_a, n_b, strip_bytes)
    strips = (n_a + e - 1) // e
    tb = (n_b + 127) // 128
    tiles = sum((min(e, n_a - s * e) + 127) // 128 * tb for s in range(strips))
    return strips, e, tiles
