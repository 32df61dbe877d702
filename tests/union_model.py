"""The union of columns as a model (no GPU, nothing of the library is imported): the contract of
kwage_group_union_columns on group_model.GroupModel's, and the table of cases tests/test_gpu_union.py runs on a device.

  union(dst, src, sets)   a union is the model's insert of the row-wise OR of the source model's member columns; within one
                          group (dst is src) it is placed at the next 16-byte boundary of the row ALSO behind an open tail --
                          the columns skipped stay what they were: pad columns.  Returns the first new column, or the error
                          code with both models untouched.  None of the planners (union_plan.hpp, insert_plan.hpp) is
                          called: tests/test_union_model.py holds the two to each other.
  CASES                   (L, source, dest, list): how the source group is built, what state the destination is in, which
                          member lists are united.  case_ops(case) gives the steps that build both groups as group_model.Op's
                          (replayed on models here and on device groups in the GPU test) and the member lists."""
import numpy as np

import group_model as gm

ERR_ARG, ERR_STATE = gm.ERR_ARG, gm.ERR_STATE
K, NH = 15, 2
LS = (0, 3, 5, 6, 10)                   # one row, fewer rows than a wave, more rows than a workgroup of 256 lanes has units
SOURCES = ("blocks", "retired", "kib")
OPEN_TAILS = (1, 31, 32, 33, 127, 128, 129)
DESTS = ("fresh", "closed") + tuple("open-%d" % r for r in OPEN_TAILS) + ("emptied", "final-fresh", "final-open-33", "final-closed",
                                                                          "same-open", "same-closed", "same-final")
LISTS = ("one", "all", "129sets", "dwords", "repeat", "200sets", "unequal")
CAPACITY = {"blocks": 1400, "retired": 1400, "kib": 8300 + 1400}      # columns: the source's, and room for a union behind a pad


def union(dst, src, sets):
    """kwage_group_union_columns on the models -> the first new column in dst, or the error code (both models untouched)."""
    sets = [[int(c) for c in s] for s in sets]
    if not sets or any(not s for s in sets):
        return ERR_ARG
    if dst.L != src.L:
        return ERR_ARG
    if any(c >= src.span or not src.valid[c] for s in sets for c in s):
        return ERR_ARG
    new = np.stack([src.matrix[:, s].any(axis=1) for s in sets], axis=1)
    if dst is not src:
        return dst.insert(gm.filters_of(new))
    # within one group: as if the tail were closed -- the next 16-byte boundary of the row
    was_open, dst.tail_open = dst.tail_open, False
    first = dst.insert(gm.filters_of(new))
    if first < 0:
        dst.tail_open = was_open
    return first


def cases():
    out = []
    for li, lst in enumerate(LISTS):                  # every list at every filter length
        for Li, L in enumerate(LS):
            out.append((L, SOURCES[(li + Li) % 3], DESTS[(5 * li + Li) % len(DESTS)], lst))
    for di, dest in enumerate(DESTS):                 # every destination with the two lists that make the most units and the most uneven lanes
        for lst in ("129sets", "unequal", "one"):
            case = (6 if lst != "one" else 5, SOURCES[di % 3], dest, lst)
            if case not in out:
                out.append(case)
    for case in ((6, "blocks", "open-127", "200sets"), (10, "kib", "open-129", "200sets")):      # three units, the first and the last partly
        if case not in out:
            out.append(case)
    return out


CASES = cases()


def case_id(case):
    return "L%d-%s-%s-%s" % case


def _random_image(rng, nrows, nf):
    """A file-like block: whole bytes of random bits, the pad bits of the last byte garbage (all set)."""
    image = np.packbits(rng.random((nrows, 8 * ((nf + 7) // 8))) < 0.3, axis=1, bitorder="little")
    if nf % 8:
        image[:, -1] |= (0xFF << (nf % 8)) & 0xFF
    return image


def _filters(rng, L, n):
    return gm.random_filters(rng, L, n) & gm.random_filters(rng, L, n)      # density 1/4: an OR of a few stays informative


def source_ops(rng, L, source, same):
    """The steps that build the source group "S" (same: which same-group state it is left in, or None)."""
    nrows, ops = 1 << L, []
    op = lambda kind, **a: ops.append(gm.Op(kind, on="S", **a))
    if source == "blocks":
        # two ragged file-like blocks with garbage in their pad bits, then inserts behind them
        op("add_columns", image=_random_image(rng, nrows, 77), nf=77)
        op("add_columns", image=_random_image(rng, nrows, 45), nf=45)
        op("insert", filters=_filters(rng, L, 21))
    elif source == "retired":
        # a retired column with set bits left in it beside a member in the same dword (34: 33's neighbour), bits in pad columns
        op("insert", filters=_filters(rng, L, 70))
        op("retire", cols=[33, 5])
        op("set_bits", rows=np.arange(nrows), cols=np.full(nrows, 33))
        op("set_bits", rows=rng.integers(0, nrows, size=8), cols=np.full(8, 71))       # (70 .. 71: the pad behind the tail)
    else:
        # a span that crosses the 8192-column KiB step of a row
        op("insert", filters=_filters(rng, L, 8300))
    if same == "same-closed":
        op("add_columns", image=_random_image(rng, nrows, 13), nf=13)
    elif same in ("same-open", "same-final"):
        op("insert", filters=_filters(rng, L, 3))
        if same == "same-final":
            op("finalize")
    return ops


def dest_ops(rng, L, dest):
    """The steps that bring a destination group "D" into the state `dest` (none for the same-group states)."""
    nrows, ops = 1 << L, []
    op = lambda kind, **a: ops.append(gm.Op(kind, on="D", **a))
    if dest.startswith("same"):
        return ops
    if dest in ("closed", "final-closed"):
        op("add_columns", image=_random_image(rng, nrows, 70), nf=70)
    elif "open" in dest:
        op("insert", filters=gm.random_filters(rng, L, int(dest.rsplit("-", 1)[1])))
    elif dest == "emptied":
        # what a compaction of a group without valid columns leaves: span 0, the tail open at 0, the memory as it was
        op("insert", filters=gm.random_filters(rng, L, 300))
        op("retire", cols=list(range(300)))
        op("set_bits", rows=rng.integers(0, nrows, size=64), cols=rng.integers(0, 300, size=64))
        op("compact")
    if dest.startswith("final"):
        op("finalize")
    return ops


def lists_of(rng, lst, src):
    """The member lists of a case for the source model `src` (its state after source_ops)."""
    v = np.flatnonzero(src.real)
    pick = lambda n: [int(c) for c in rng.choice(v, size=n, replace=n > v.size)]
    if lst == "one":
        return [[int(v[v.size // 2])]]
    if lst == "all":
        return [[int(c) for c in v]]
    if lst == "129sets":                              # two units where the union starts on a unit's boundary, the last holding one column
        return [pick(1 + j % 3) for j in range(129)]
    if lst == "dwords":
        same_dword = [int(c) for c in v if c // 32 == v[v.size // 2] // 32]
        dwords = sorted({int(c) // 32 for c in v})
        d = [a for a, b in zip(dwords, dwords[1:]) if b == a + 1][-1]       # the last two adjacent dwords that both hold members
        adjacent = [int(c) for c in v if c // 32 in (d, d + 1)]
        return [same_dword, adjacent, [int(v[0]), int(v[-1])], [int(v[-1])], [int(v[0])]]
    if lst == "repeat":
        a, b = pick(2)
        return [[a, b, a, a], [b, b]]
    if lst == "200sets":                              # one column in 200 sets
        c = int(v[3])
        return [[c] if j % 2 else [c] + pick(1) for j in range(200)]
    assert lst == "unequal"                           # very unequal sizes within one unit
    return [pick(1), [int(c) for c in v], pick(2), pick(min(50, v.size)), pick(1), pick(17), [int(c) for c in v[::2]]]


def case_ops(case):
    """-> (ops that build the groups, name of the destination ("S" within one group), capacities {"S": .., "D": ..})."""
    L, source, dest, lst = case
    rng = np.random.default_rng([L, SOURCES.index(source), DESTS.index(dest), LISTS.index(lst)])
    same = dest if dest.startswith("same") else None
    ops = source_ops(rng, L, source, same) + dest_ops(rng, L, dest)
    return ops, ("S" if same else "D"), {"S": CAPACITY[source], "D": 1400}, rng


def fresh_models(case, capacities):
    return {name: gm.GroupModel(case[0], gm.stride_of(cap)) for name, cap in capacities.items()}


def reveal_ops(model, name):
    """One-column blocks of zeros behind everything until the row is full: they bring every byte of the row up to the
    stride into the span, where read_rows shows it (a group that is not finalized only)."""
    ops = []
    next_byte = model.next_byte
    while (next_byte + 15) // 16 * 16 < model.stride:
        ops.append(gm.Op("add_columns", on=name, image=np.zeros((model.nrows, 1), dtype=np.uint8), nf=1))
        next_byte = (next_byte + 15) // 16 * 16 + 1
    return ops
