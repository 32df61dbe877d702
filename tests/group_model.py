"""A model of a live dense group (no GPU, nothing of the library is imported at module level): the expected state of a
resident group under every mutator of include/kwage_amd.h, a seeded generator of operation sequences, and the numpy /
oracle helpers that compare a device group with an expected matrix.

  GroupModel      the state: every bit of every row up to the row stride, the valid mask, next_byte, the tail, finalized.
                  One method per mutator (add_columns, insert, retire, set_bits, compact, finalize); each returns what the C
                  ABI call must return -- the first column, (column map, stats), 0 -- or the error code, the state then
                  untouched.  fold(L2) returns (a NEW model, the stats of kwage_group_fold) and leaves this one alone
                  (tests/family_model.py walks over several models).  The rules are restated from the header's text; none
                  of the planners (insert_plan.hpp, compact_plan.hpp, fold_plan.hpp) is called: tests/test_group_model.py
                  and tests/test_family_model.py compare the two, tests/test_gpu_group_model.py and
                  tests/test_gpu_family_model.py replay the sequences on the device and compare after every step.
  sequence        (seed, shape) -> Sequence: about 45 operations of a seeded walk on the model, the planned refusals and the
                  checkpoints (where the GPU test runs every search form) included, and the seed's queries.
  Image, check_rows, check_all_forms, oracle_counts, oracle_hits, state_of, same_state ...
                  what tests/test_gpu_live_insert.py compares a group with (they lived there; it imports them back).
                  A GroupModel offers .bits, .real, .span and .packed() as an Image does.

What the model says where the header leaves room:
  - the matrix is kept up to the STRIDE, not the span: bits above the span exist in memory (pad bits a block's last byte
    brought, bits set_bits planted in pad columns) and come into sight again when the span grows over them;
  - a compaction with nothing to close (every column below the open tail valid) launches nothing, so bits planted in the
    pad columns between the tail and the span stay until the next insert overwrites them; one with m == 0 launches
    nothing either, the span becomes 0 and the memory keeps what it held;
  - otherwise a compaction rewrites whole 16-byte units up to the end of the unit the old span ends in: zero from column m
    to there."""
import ctypes as C

import numpy as np

ERR_ARG, ERR_STATE = -1, -6

# (L, capacity in columns, k, num_hash): the smallest shapes at which each edge exists
SHAPES = [(0, 300, 5, 1), (3, 300, 15, 2), (5, 300, 15, 3), (8, 1100, 21, 2), (10, 8500, 31, 5), (9, 8500, 31, 1)]
WIDE_SHAPES = SHAPES[4:]          # rows of more than a KiB: the wide gather kernels, the truncated count walk


def stride_of(capacity):
    """A group's row stride in bytes: its capacity rounded up to whole bytes, then to 128 bytes."""
    return ((capacity + 7) // 8 + 127) // 128 * 128


# ----------------------------------------------------------------------------------------------------------------------
# the numpy side
# ----------------------------------------------------------------------------------------------------------------------

def random_filters(rng, L, n):
    """uint8 [n, max(1, 2^L / 8)] at density 1/2; for L < 3 the bits at and beyond 2^L are garbage (to be ignored)."""
    return rng.integers(0, 256, size=(n, max(1, (1 << L) // 8)), dtype=np.uint8)


def columns_of(filters, L):
    """bool [2^L, n]: unpackbits, then the transpose."""
    return np.unpackbits(filters, axis=1, bitorder="little")[:, :1 << L].T.astype(bool)


def filters_of(columns):
    """The inverse: bool [2^L, n] -> uint8 [n, max(1, 2^L / 8)], LSB first (for L < 3 the bits at and beyond 2^L are zero)."""
    return np.packbits(np.ascontiguousarray(columns.T), axis=1, bitorder="little")


class Image:
    """The expected matrix: bool [2^L, span] and the real columns."""

    def __init__(self, L):
        self.bits = np.zeros((1 << L, 0), dtype=bool)
        self.real = np.zeros(0, dtype=bool)

    def put(self, first, cols):
        span = (first + cols.shape[1] + 7) // 8 * 8
        if span > self.bits.shape[1]:
            grow = span - self.bits.shape[1]
            self.bits = np.concatenate([self.bits, np.zeros((self.bits.shape[0], grow), dtype=bool)], axis=1)
            self.real = np.concatenate([self.real, np.zeros(grow, dtype=bool)])
        assert not self.real[first:first + cols.shape[1]].any()
        self.bits[:, first:first + cols.shape[1]] = cols
        self.real[first:first + cols.shape[1]] = True

    def retire(self, c):
        assert self.real[c]
        self.bits[:, c] = False
        self.real[c] = False

    @property
    def span(self):
        return self.bits.shape[1]

    def packed(self):
        return np.packbits(self.bits, axis=1, bitorder="little")


def check_rows(g, image, rows=None):
    rows = np.arange(image.bits.shape[0]) if rows is None else rows
    assert g.column_span == image.span and g.row_bytes == image.span // 8 and g.num_columns == int(image.real.sum())
    got = g.read_rows(rows)
    assert np.array_equal(got, image.packed()[rows]), np.argwhere(got != image.packed()[rows])[:5]


def random_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def state_of(g, nrows):
    return (g.column_span, g.num_columns, g.row_bytes, g.real_columns().copy(), g.read_rows(np.arange(nrows)) if g.row_bytes else None)


def same_state(a, b):
    return a[:3] == b[:3] and np.array_equal(a[3], b[3]) and (a[4] is None) == (b[4] is None) and (a[4] is None or np.array_equal(a[4], b[4]))


# ----------------------------------------------------------------------------------------------------------------------
# the oracle side: every search form's expected result from the image
# ----------------------------------------------------------------------------------------------------------------------

def oracle_counts(oracle, image, k, nh, L, queries):
    """(int64 [n, span] num_match of every column, uint32 [n] distinct k-mers)."""
    packed = np.ascontiguousarray(image.packed())
    counts = np.zeros((len(queries), image.span), dtype=np.int64)
    nk = []
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, k)
        nk.append(len(kmers))
        if len(kmers):
            for c, m in oracle.search_image(packed, packed.shape[1], k, nh, L, image.span, kmers, 1e-12)[0]:
                counts[q, c] = m
    return counts, np.asarray(nk, dtype=np.uint32)


def oracle_hits(oracle, image, k, nh, L, queries, t):
    """[(query, column, num_match)] of the real columns, by (query, column): the oracle's own threshold search."""
    packed = np.ascontiguousarray(image.packed())
    out = []
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, k)
        if len(kmers):
            hits, _ = oracle.search_image(packed, packed.shape[1], k, nh, L, image.span, kmers, float(np.float32(t)))
            out.extend((q, c, m) for c, m in hits if image.real[c])
    return out


def check_all_forms(ka, oracle, g, image, ctx, k, nh, L, queries, fs_columns, twin=None, topk=5):
    """Every search form of the group against the oracle on the image (and against `twin`, a group that must answer the
    same).  Returns the threshold search's records at t = 1 and 0.8 for the caller to compare across states."""
    from kwage_amd.native import lib
    counts, nk = oracle_counts(oracle, image, k, nh, L, queries)
    real = image.real
    assert np.array_equal(g.real_columns(), real)
    b = ka.Batch(ctx, queries)
    kept = {}
    try:
        for t in (1.0, 0.8):
            exp = oracle_hits(oracle, image, k, nh, L, queries, t)
            for flags in (0, ka.SEARCH_EARLY_EXIT):
                r = g.search(b, t, flags)
                got = [tuple(h) for h in r.hits.tolist()]
                assert np.array_equal(r.num_query_kmer, nk)
                assert got == exp, (t, flags, got[:5], exp[:5])
                assert all(real[c] for _, c, _ in got)
                if twin is not None:
                    assert [tuple(h) for h in twin.search(b, t, flags).hits.tolist()] == got
            kept[t] = exp
            # presence: the same (query, column) pairs as a bitmap
            floors = np.array([oracle.query_threshold(float(np.float32(t)), int(n)) for n in nk], dtype=np.int64)
            want = real[None, :] & (counts >= floors[:, None]) & (nk[:, None] > 0)
            assert {(q, c) for q, c in np.argwhere(want).tolist()} == {(q, c) for q, c, _ in exp}
            p = g.search_presence(b, t)
            assert np.array_equal(p.unpack()[:, :image.span], want), t
            if twin is not None:
                assert np.array_equal(twin.search_presence(b, t).bits, p.bits)
        # top-k at floor 0: (score descending, column ascending), cut at k, listed by (query, column)
        exp_top = []
        for q in range(len(queries)):
            if nk[q]:
                best = sorted((c for c in range(image.span) if real[c]), key=lambda c: (-counts[q, c], c))[:topk]
                exp_top.extend((q, c, int(counts[q, c])) for c in sorted(best))
        r = g.search_topk(b, topk)
        assert [tuple(h) for h in r.hits.tolist()] == exp_top
        if twin is not None:
            assert [tuple(h) for h in twin.search_topk(b, topk).hits.tolist()] == exp_top
        # dense scores
        want = np.where(real[None, :] & (nk[:, None] > 0), counts, 0).astype(np.uint32)
        s = g.search_scores(b)
        assert np.array_equal(s.scores, want)
        if twin is not None:
            assert np.array_equal(twin.search_scores(b).scores, want)
    finally:
        b.close()
    # column bits, and the filter search with the listed columns as the questions
    bits = np.where(real, image.bits.sum(axis=0), 0).astype(np.uint32)
    assert np.array_equal(g.column_bits(), bits)
    if fs_columns:
        fs = ka.FilterSet.from_columns(g, fs_columns)
        try:
            shared = np.stack([np.where(real, (image.bits & image.bits[:, c:c + 1]).sum(axis=0), 0) for c in fs_columns]).astype(np.uint32)
            assert np.array_equal(g.search_filter_scores(fs).scores, shared)
            assert np.array_equal(fs.bit_counts(), bits[fs_columns])
            if twin is not None:
                assert np.array_equal(twin.search_filter_scores(fs).scores, shared)
        finally:
            fs.close()
    for c in np.flatnonzero(~real)[:3].tolist():
        h = C.c_void_p()
        cols = np.array([c], dtype=np.uint64)
        assert lib().kwage_filterset_from_columns(g._h, cols.ctypes.data, 1, C.byref(h)) == ERR_ARG       # a pad column is refused
    return kept


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------

class GroupModel:
    """The expected state of a dense group of 2^L rows, `stride_bytes` apart."""

    def __init__(self, L, stride_bytes):
        self.L, self.nrows, self.stride = L, 1 << L, stride_bytes
        self.matrix = np.zeros((self.nrows, 8 * stride_bytes), dtype=bool)      # every bit of a row, up to the stride
        self.valid = np.zeros(8 * stride_bytes, dtype=bool)
        self.next_byte, self.tail_open, self.tail_column, self.finalized = 0, False, 0, False

    # what an Image offers
    span = property(lambda self: 8 * self.next_byte)
    bits = property(lambda self: self.matrix[:, :self.span])
    real = property(lambda self: self.valid[:self.span])
    num_columns = property(lambda self: int(self.valid.sum()))

    def packed(self):
        return np.packbits(self.bits, axis=1, bitorder="little")

    def copy(self):
        m = GroupModel.__new__(GroupModel)
        m.__dict__.update(self.__dict__)
        m.matrix, m.valid = self.matrix.copy(), self.valid.copy()
        return m

    def same(self, other):
        return (self.next_byte, self.tail_open, self.tail_column, self.finalized) == (other.next_byte, other.tail_open, other.tail_column, other.finalized) \
            and np.array_equal(self.valid, other.valid) and np.array_equal(self.matrix, other.matrix)

    # -- kwage_group_add_columns: a block starts at the next 16-byte boundary of the row and closes the tail; its last byte is
    #    copied whole, the bits beyond num_filter with it; refused after finalize
    def add_columns(self, image, nf):
        if self.finalized:
            return ERR_STATE
        if nf == 0:
            return ERR_ARG
        start, width = (self.next_byte + 15) // 16 * 16, (nf + 7) // 8
        if start + width > self.stride:
            return ERR_ARG
        self.matrix[:, 8 * start:8 * (start + width)] = np.unpackbits(np.ascontiguousarray(image[:, :width]), axis=1, bitorder="little").astype(bool)
        self.valid[8 * start:8 * start + nf] = True
        self.next_byte, self.tail_open = start + width, False
        return 8 * start

    # -- the live insert: at the very next column behind an open tail, else at the next 16-byte boundary; the call owns
    #    everything from its first column to the end of the last 32-bit word it touches -- bits below first % 32 are kept,
    #    bits at and above the new tail are zero
    def insert(self, filters):
        n = len(filters)
        if n == 0:
            return ERR_ARG
        first = self.tail_column if self.tail_open else (self.next_byte + 15) // 16 * 16 * 8
        if first > 8 * self.stride or n > 8 * self.stride - first:
            return ERR_ARG
        word_end = ((first + n - 1) // 32 + 1) * 32
        self.matrix[:, first:first + n] = columns_of(filters, self.L)
        self.matrix[:, first + n:word_end] = False
        self.valid[first:first + n] = True
        self.tail_column, self.tail_open, self.next_byte = first + n, True, (first + n + 7) // 8
        return first

    # -- retire: columns may repeat; a column at or beyond the span or a pad column refuses the whole call
    def retire(self, cols):
        cols = [int(c) for c in cols]
        for c in cols:
            if c >= self.span or not self.valid[c]:
                return ERR_ARG
        if cols:
            self.matrix[:, cols] = False
            self.valid[cols] = False
        return 0

    # -- set_bits: any column below the span, real or dead
    def set_bits(self, rows, cols):
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        if rows.size and ((rows >= self.nrows).any() or (cols >= self.span).any()):
            return ERR_ARG
        self.matrix[rows, cols] = True
        return 0

    # -- compaction: the m valid columns become columns 0 .. m - 1 in their order, the tail opens at m
    def compact(self):
        span = self.span
        v = self.valid[:span].copy()
        m = int(v.sum())
        new_column = np.where(v, np.cumsum(v) - 1, -1).astype(np.int64)
        idx = np.flatnonzero(v)
        runs = int(1 + np.count_nonzero(np.diff(idx) != 1)) if m else 0
        dead = np.flatnonzero(~v)
        p = int(dead[0]) if dead.size else span
        nothing_to_close = p >= (min(self.tail_column, span) if self.tail_open else span)
        # the 16-byte units of a row that are rewritten: none, or from the one that holds the first dead column to the old span's last
        first_unit, units = (p // 128, (span + 127) // 128 - p // 128) if m and not nothing_to_close else (0, 0)
        if units:
            survivors = self.matrix[:, :span][:, v]
            self.matrix[:, :m] = survivors
            self.matrix[:, m:(span + 127) // 128 * 128] = False
        self.valid[:span] = False
        self.valid[:m] = True
        self.next_byte, self.tail_column, self.tail_open = (m + 7) // 8, m, True
        return new_column, {"span_before": span, "span_after": 8 * self.next_byte, "columns": m, "runs": runs, "first_unit": first_unit, "units": units,
                            "nothing_to_close": bool(nothing_to_close)}

    def finalize(self):
        self.finalized = True
        return 0

    # -- kwage_group_fold: a NEW group of 2^L2 rows at the same stride; with U = ceil(row_bytes / 16), bytes [0, 16 U) of
    #    row r' are the OR of the same bytes of the rows r' + j * 2^L2, everything from 16 U to the stride is zero; the
    #    column layout (valid mask, next_byte, the tail) and finalized are this group's, which is not changed
    def fold(self, L2):
        if not 0 <= L2 < self.L:
            return ERR_ARG
        units = (self.next_byte + 15) // 16
        m = GroupModel(L2, self.stride)
        m.matrix[:, :128 * units] = self.matrix[:, :128 * units].reshape(1 << (self.L - L2), 1 << L2, 128 * units).any(axis=0)
        m.valid = self.valid.copy()
        m.next_byte, m.tail_open, m.tail_column, m.finalized = self.next_byte, self.tail_open, self.tail_column, self.finalized
        return m, {"log_2_before": self.L, "log_2_after": L2, "units_per_row": units, "bytes_read": 16 * units << self.L,
                   "bytes_written": 16 * units << L2}

    def room(self):
        """Columns a live insert (or a copy) could still take."""
        return 8 * self.stride - (self.tail_column if self.tail_open else (self.next_byte + 15) // 16 * 16 * 8)

    def apply(self, op):
        """One Op of a sequence on this model -> what the call returns."""
        if op.kind == "add_columns":
            return self.add_columns(op.image, op.nf)
        if op.kind == "insert":
            return self.insert(op.filters)
        if op.kind == "retire":
            return self.retire(op.cols)
        if op.kind == "set_bits":
            return self.set_bits(op.rows, op.cols)
        if op.kind == "compact":
            return self.compact()
        if op.kind == "finalize":
            return self.finalize()
        assert op.kind == "checkpoint", op.kind
        return 0


# ----------------------------------------------------------------------------------------------------------------------
# operation sequences
# ----------------------------------------------------------------------------------------------------------------------

class Op:
    """One step of a sequence: kind, its arguments as attributes, `result` (what the model returned when the sequence was
    made) and `tags` (what the ledger of tests/test_group_model.py counts)."""

    def __init__(self, kind, tags=(), **args):
        self.kind, self.tags, self.result = kind, set(tags), None
        self.__dict__.update(args)

    def refused(self):
        return isinstance(self.result, int) and self.result < 0

    def __repr__(self):
        return "Op(%s%s)" % (self.kind, "".join(" " + t for t in sorted(self.tags)))


class Sequence:
    def __init__(self, seed, shape, stride, ops, queries, fill_query):
        self.seed, self.shape, self.stride, self.ops, self.queries, self.fill_query = seed, shape, stride, ops, queries, fill_query
        self.finalizes = any(op.kind == "finalize" for op in ops)


INSERT_FORMS = ("host", "device", "files")
RESIDUES = (1, 7, 8, 31, 0)           # first columns mod 32 that the inserts are steered to
LONG = 620                            # bases of the two long queries


def _mutate(seq, positions):
    s = list(seq)
    for p in positions:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


class _Walk:
    """The seeded walk: it carries the model along, so that every operation is chosen for the state it meets."""

    def __init__(self, seed, shape):
        import kwage_oracle as oracle
        oracle.build()
        self.oracle, self.seed, self.shape = oracle, seed, shape
        self.L, self.cap, self.k, self.nh = shape
        self.rng = np.random.default_rng([seed, self.L, self.cap, self.k, self.nh])
        self.m = GroupModel(self.L, stride_of(self.cap))
        self.ops, self.n_inserts, self.touched, self.retired = [], 0, set(), set()
        self.wide = shape in WIDE_SHAPES
        rng, k = self.rng, self.k
        # samples: short ones whose exact filters fill about 0.3 of the rows, so that a random query misses them
        glen = k + min(max(int(0.35 * (1 << self.L) / self.nh), 2), 120) - 1
        self.genomes = [random_dna(rng, glen) for _ in range(6)]
        self.genome_filters = np.stack([oracle.bloom_bits_from_sequences([s], k, self.nh, self.L) for s in self.genomes])
        g = self.genomes
        long1 = random_dna(rng, LONG)
        # 13 queries: substrings of inserted samples, the same with a base changed (one k-mer lost: they pass at 0.8, not at
        # 1), two long ones (the second the first with three bases changed), random ones, one of exactly k bases (one
        # k-mer: the threshold at 0.8 is 0), one shorter than k, one with an N
        self.queries = [g[0], g[1][1:], g[2][:-1], _mutate(g[0], [glen - 1]), _mutate(g[1][1:], [glen - 2]), _mutate(g[3], [0]),
                        long1, _mutate(long1, [200, 201, 450]), random_dna(rng, k + 12), random_dna(rng, k + 3), random_dna(rng, k),
                        random_dna(rng, k - 1), g[4][:k + 1] + "N" + g[5]]
        self.fill_query = 6
        self.next_genome = 0

    # -- emitting
    def emit(self, kind, tags=(), **args):
        op = Op(kind, tags, **args)
        before = self.m.copy() if kind in ("retire", "compact") else None
        op.result = self.m.apply(op)
        if kind == "insert" and not op.refused():
            self.n_inserts += 1
            lo, hi = op.result, op.result + len(op.filters)
            self.touched = {c for c in self.touched if c < lo}
            self.retired = {c for c in self.retired if c < lo}
            for edge in (1024, 8192):
                if lo < edge < hi:
                    op.tags.add("cross%d" % edge)
            op.tags.add("first%%32=%d" % (lo % 32))
        if kind == "retire" and not op.refused():
            gone = set(int(c) for c in op.cols)
            self.touched -= gone
            self.retired |= gone
            v0, v1 = before.valid[:before.span], self.m.valid[:before.span]
            for u in range(0, before.span, 128):
                if v0[u:u + 128].any() and not v1[u:u + 128].any() and u + 128 <= before.span:
                    op.tags.add("empties_unit")
        if kind == "compact":
            new = op.result[0]
            self.touched = {int(new[c]) for c in self.touched if new[c] >= 0}
            self.retired = set()
            if op.result[1]["nothing_to_close"]:
                op.tags.add("nothing_to_close")
                if before.matrix[:, before.tail_column:before.span].any():
                    op.tags.add("order2")
        self.ops.append(op)
        return op

    def room(self):
        first = self.m.tail_column if self.m.tail_open else (self.m.next_byte + 15) // 16 * 16 * 8
        return 8 * self.m.stride - first

    def filters(self, n, with_genomes=True):
        """n filters at density 1/4, every fifth call's first ones the exact filters of samples."""
        f = random_filters(self.rng, self.L, n) & random_filters(self.rng, self.L, n)
        if with_genomes:
            for i in range(min(n, 2)):
                f[i] = self.genome_filters[self.next_genome % len(self.genomes)]
                self.next_genome += 1
        return f

    def insert(self, n, tags=(), reserve=80):
        n = min(n, self.room() - reserve)
        if n < 1:
            return None
        form = INSERT_FORMS[(self.n_inserts + self.seed) % 3]
        if form == "files" and n > 64:
            form = "host"
        return self.emit("insert", tags, filters=self.filters(n), form=form)

    def real_columns(self):
        return np.flatnonzero(self.m.real)

    def checkpoint(self, tags=()):
        real = self.real_columns()
        fs = [int(c) for c in self.rng.choice(real, size=min(2, real.size), replace=False)] if real.size else []
        extra = sorted(self.touched - set(fs)) or [int(c) for c in real if int(c) not in fs]
        if extra:
            fs.append(extra[0])
        self.emit("checkpoint", tags, fs=fs, search=self.m.finalized)

    # -- the pieces
    def block(self, lo, hi):
        nf = int(self.rng.integers(lo, hi))
        nf += nf % 8 == 0                                       # ragged: no multiple of 8
        width = (nf + 7) // 8
        if (self.m.next_byte + 15) // 16 * 16 + width > self.m.stride - 16:
            return
        image = np.packbits(self.rng.random((self.m.nrows, 8 * width)) < 0.25, axis=1, bitorder="little")      # (pad bits: garbage)
        self.emit("add_columns", image=image, nf=nf)

    def set_bits(self, cols, tags, n=6):
        cols = np.asarray(cols, dtype=np.int64)
        pick = self.rng.choice(cols, size=n)
        rows = self.rng.integers(0, self.m.nrows, size=n)
        op = self.emit("set_bits", tags, rows=rows, cols=pick)
        self.touched |= {int(c) for c in pick if self.m.valid[c]}
        return op

    def ragged_tail(self):
        """An open tail that is no multiple of 8: pad columns between the tail and the span exist."""
        if not (self.m.tail_open and self.m.tail_column % 8):
            n = 13 if (self.m.tail_column + 13) % 8 or not self.m.tail_open else 14
            self.insert(n)
        return self.m.tail_open and self.m.tail_column % 8 != 0

    def steered_inserts(self):
        """Two inserts, the first sized so that the second starts at a wanted residue mod 32."""
        if not self.m.tail_open:
            self.insert(int(self.rng.integers(2, 41)))
        want = RESIDUES[(self.seed + self.n_inserts) % len(RESIDUES)]
        n = (want - self.m.tail_column) % 32
        self.insert(n if n >= 2 else n + 32)
        self.insert(int(self.rng.integers(2, 41)))

    def retire(self, how):
        m, real = self.m, self.real_columns()
        if real.size < 3:
            return
        cols = None
        if how in ("word", "unit"):
            w = 32 if how == "word" else 128
            full = [u for u in range(0, m.span - w + 1, w) if m.valid[u:u + w].all()]
            if full:
                u = full[int(self.rng.integers(len(full)))]
                cols = list(range(u, u + w))
        elif how == "last":
            cols = [int(real[-1])]
            how = "last" if m.tail_open and real[-1] == m.tail_column - 1 else "single"
        elif how == "twice":
            a, b = self.rng.choice(real, size=2, replace=False)
            cols = [int(a), int(b), int(a)]
        if cols is None:
            how, cols = "single", [int(self.rng.choice(real))]
        self.emit("retire", ["retire_" + how], cols=cols)

    # -- the planned refusals: each is checked by the driver to have changed nothing
    def refuse_capacity(self):
        n = self.room() + 1
        self.emit("insert", ["refuse_capacity"], filters=self.filters(n, with_genomes=False), form=("host", "device")[self.seed % 2])

    def refuse_pad_retire(self):
        real, dead = self.real_columns(), np.flatnonzero(~self.m.real)
        if real.size and dead.size:
            self.emit("retire", ["refuse_pad"], cols=[int(real[0]), int(self.rng.choice(dead))])
        elif real.size:
            self.emit("retire", ["refuse_beyond_span"], cols=[int(real[0]), self.m.span])

    def refuse_add(self):
        image = np.packbits(self.rng.random((self.m.nrows, 8)) < 0.5, axis=1, bitorder="little")
        self.emit("add_columns", ["refuse_add"], image=image, nf=5)

    def refuse_set_at_span(self):
        self.emit("set_bits", ["refuse_set_at_span"], rows=np.array([0, 0]), cols=np.array([max(self.m.span - 1, 0), self.m.span]))

    # -- the walk
    def run(self):
        rng, m = self.rng, self.m
        finalizes = self.seed % 4 != 3
        # before finalize: a first block wide enough to hold a whole 16-byte unit, then the rest in random order
        self.block(7000, 7150) if self.wide else self.block(150, 200)      # (wide: the large insert below crosses column 8192)
        pre = ["insert", "set_bits", "block", "retire", "insert", "set_bits"] + (["block"] if self.seed % 2 == 0 else [])
        rng.shuffle(pre)
        last_block = max(i for i, p in enumerate(pre) if p == "block")
        at = int(rng.integers(last_block + 1, len(pre) + 1)) if finalizes else len(pre) + 1
        for i, p in enumerate(pre):
            if i == at:
                self.emit("finalize")
            if p == "insert":
                self.insert(int(rng.integers(1, 30)))
            elif p == "block":
                self.block(13, 70)
            elif p == "set_bits":
                self.set_bits(np.arange(m.span), ["set_any"])
            else:
                real = self.real_columns()
                self.emit("retire", ["retire_pre"], cols=[int(c) for c in rng.choice(real[real >= 128], size=3, replace=False)])
        if at == len(pre):
            self.emit("finalize")
        if finalizes and self.seed % 2:
            self.emit("finalize")                                # (a second finalize call changes nothing)
        self.checkpoint()
        # afterwards: the deck, in random order; the one insert of more than 1024 filters first, while there is room
        if 8 * m.stride >= 2048:
            self.insert(int(rng.integers(1030, 1100)), ["insert_big"], reserve=250 if not self.wide else 500)
        deck = ["insert1", "steered", "steered", "retire_single", "retire_word", "retire_unit", "retire_last", "retire_twice",
                "order1", "set_retired", "set_pad", "order2", "compact_twice", "refuse_capacity", "refuse_set_at_span"]
        deck += ["refuse_add"] if finalizes else []
        deck += ["order3"] if self.wide else []
        rng.shuffle(deck)
        for item in deck:
            if item == "insert1":
                self.checkpoint()                                # (column_bits() before and after: the cache must not outlive the insert)
                self.insert(1, ["cache_insert"] if m.finalized else [])
                self.checkpoint()
            elif item == "steered":
                self.steered_inserts()
            elif item == "retire_single":
                self.retire("single")
                self.refuse_pad_retire()
            elif item == "retire_twice":
                self.checkpoint()                                # (... nor the retire)
                self.retire("twice")
                if m.finalized:
                    self.ops[-1].tags.add("cache_retire")
                self.checkpoint()
            elif item.startswith("retire_"):
                self.retire(item[7:])
            elif item == "order1":
                # column_bits() at a checkpoint, set_bits on real columns, column_bits() again
                self.checkpoint()
                self.set_bits(self.real_columns(), ["set_real", "order1"] if m.finalized else ["set_real"], n=9)
                self.checkpoint()
            elif item == "set_retired":
                gone = sorted(c for c in self.retired if c < m.span and not m.valid[c])
                if not gone:
                    self.retire("single")
                    gone = sorted(c for c in self.retired if c < m.span and not m.valid[c])
                if gone:
                    self.set_bits(gone, ["set_retired"])
            elif item == "set_pad":
                if self.ragged_tail():
                    self.set_bits(np.arange(m.tail_column, m.span), ["set_pad"], n=4)
            elif item == "order2":
                # a compaction directly after an insert, nothing retired in between, bits planted above the tail
                self.emit("compact")
                self.insert(13 if (m.tail_column + 13) % 8 else 14)
                if m.tail_column % 8:
                    self.set_bits(np.arange(m.tail_column, m.span), ["set_pad"], n=4)
                self.emit("compact", ["compact_after_insert"])
                self.insert(int(rng.integers(2, 20)), ["insert_after_compact"])
            elif item == "compact_twice":
                self.retire("single")
                self.checkpoint()                                # (... nor the compaction, which renumbers the columns)
                self.emit("compact", ["cache_compact"] if m.finalized else [])
                self.checkpoint()
                self.emit("compact", ["compact_twice"])
                self.insert(int(rng.integers(2, 20)), ["insert_after_compact"])
            elif item == "order3":
                # the densest real column filled in exactly the rows the first long query addresses: a column denser
                # than anything the last density probe saw, and the searches follow at once
                real = self.real_columns()
                c = int(real[np.argmax(m.bits[:, real].sum(axis=0))])
                rows = np.unique(self.oracle.row_indices(self.oracle.unique_kmers(self.queries[self.fill_query], self.k), self.k, self.nh, self.L))
                self.emit("set_bits", ["set_real", "order3"] if m.finalized else ["set_real"], rows=rows, cols=np.full(rows.size, c))
                self.touched.add(c)
                self.checkpoint(["after_order3"])
            else:
                getattr(self, item)()
        # the end: everything closed up, the samples the queries were cut from in again, the last checkpoint
        self.emit("compact")
        f = self.filters(min(12, self.room() - 8), with_genomes=False)
        f[:6] = self.genome_filters
        self.emit("insert", ["insert_after_compact"], filters=f, form=INSERT_FORMS[self.seed % 3])
        self.checkpoint(["last"])
        return Sequence(self.seed, self.shape, m.stride, self.ops, self.queries, self.fill_query)


def sequence(seed, shape):
    """The operations of (seed, shape): deterministic, host only."""
    return _Walk(seed, tuple(shape)).run()


def default_cases(n_seeds=12):
    """[(seed, shape)]: the seeds spread over the six shapes, seed s on shape s % 6."""
    return [(s, SHAPES[s % len(SHAPES)]) for s in range(n_seeds)]
