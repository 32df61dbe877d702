"""The contract of the overlap matrix (include/kwage_amd.h: kwage_group_column_overlaps) in numpy, with none of the
planners: unpack the bits, zero the dead columns, M_a.T @ M_b in int64.  And the lists and shapes the device tests walk."""
import numpy as np

K, NH = 31, 3
SENTINEL = -0x21524111           # 0xDEADBEEF as int32

LIST_KINDS = ("aligned", "shifted", "reversed", "shuffle", "repeat", "mixed")
COUNTS = (1, 31, 32, 33, 127, 128, 129, 300)
PAIR_COUNTS = (1, 33, 129, 300)
ROW_LOGS = (0, 3, 5, 6, 10, 14)
SPLITS = (0, 1, 2, 3, 8)


def overlaps(bits_a, valid_a, cols_a, bits_b, valid_b, cols_b):
    """uint32 [n_a, n_b]: cell (i, j) = rows in which column cols_a[i] of a and column cols_b[j] of b are both set;
    bits_x bool [rows, >= span], valid_x bool [>= span]; cols_x None = every column of the span (len(valid_x)); dead
    columns count nothing, whatever bits they hold."""
    def side(bits, valid, cols):
        cols = np.arange(len(valid)) if cols is None else np.asarray(cols, dtype=np.int64)
        return (bits[:, cols] & valid[cols][None, :]).astype(np.int64)
    a, b = side(bits_a, valid_a, cols_a), side(bits_b, valid_b, cols_b)
    return ((a.T @ b) & 0xFFFFFFFF).astype(np.uint32)


def overlaps_loop(bits_a, valid_a, cols_a, bits_b, valid_b, cols_b):
    """The same, bit by bit."""
    cols_a = range(len(valid_a)) if cols_a is None else cols_a
    cols_b = range(len(valid_b)) if cols_b is None else cols_b
    out = np.zeros((len(cols_a), len(cols_b)), dtype=np.uint32)
    for i, ca in enumerate(cols_a):
        for j, cb in enumerate(cols_b):
            n = 0
            if valid_a[ca] and valid_b[cb]:
                for r in range(bits_a.shape[0]):
                    n += 1 if bits_a[r, ca] and bits_b[r, cb] else 0
            out[i, j] = n
    return out


def of_models(ma, cols_a, mb=None, cols_b=None):
    """overlaps() of two tests/group_model.py GroupModels (mb None: the symmetric form)."""
    if mb is None:
        mb, cols_b = ma, cols_a
    return overlaps(ma.bits, ma.real, cols_a, mb.bits, mb.real, cols_b)


def blocks_of(cols, span):
    """(straight, gathered) blocks of 32 a list is cut into, as the header defines them."""
    if cols is None:
        return (span + 31) // 32, 0
    s = g = 0
    for i in range(0, len(cols), 32):
        b = [int(c) for c in cols[i:i + 32]]
        if len(b) == 32 and b[0] % 32 == 0 and b == list(range(b[0], b[0] + 32)):
            s += 1
        else:
            g += 1
    return s, g


def tiles_of(n_a, n_b, symmetric):
    ta, tb = (n_a + 127) // 128, (n_b + 127) // 128
    return ta * (ta + 1) // 2 if symmetric else ta * tb


def list_of(rng, kind, valid, n=None):
    """A list of live columns of `valid` (bool per column of the span) of one of LIST_KINDS; n columns where the kind
    leaves the count open."""
    live = np.flatnonzero(valid)
    # the longest run of live columns that starts at a multiple of 32
    starts = [s for s in range(0, len(valid) - 63, 32) if valid[s:s + 65].all()]
    if kind == "aligned":
        s = starts[0]
        return np.arange(s, s + 64)
    if kind == "shifted":
        s = starts[0]
        return np.arange(s + 1, s + 65)
    if kind == "reversed":
        return live[::-1][:n or 70].copy()
    if kind == "shuffle":
        return rng.permutation(live)[:n or 129]
    if kind == "repeat":
        c = rng.permutation(live)[:5]
        return np.array([c[0], c[1], c[0], c[2], c[0], c[0], c[3], c[4], c[1]])
    assert kind == "mixed", kind
    s = starts[0]
    return np.concatenate([np.arange(s, s + 32), rng.permutation(live)[:32], np.arange(s + 32, s + 64), live[:1]])
