"""A family of live groups as a model (no GPU, nothing of the library is imported): named group_model.GroupModel's, at most
five alive at a time, under group_model's mutators (each with on=<name>) and the calls that make one group from another:

  fold        GroupModel.fold of `src` at `L2` under a new name (kwage_group_fold, Group.fold)
  copy        copy_model.copy between two groups of equal parameters (kwage_group_copy_columns, Group.copy_columns_from);
              groups whose filter lengths differ -- a source and its own fold -- refuse it
  union       union_model.union of member lists `sets` of `src` into `on`, which may be the same name
              (kwage_group_union_columns, Group.union_columns); refused between filter lengths as the copy is.  sequence()
              makes none: tests/union_walk.py walks with it
  new         a group created natively at a given filter length: the partner a fold copies to and from
  close       the group is gone; whatever was folded or copied from it lives on
  checkpoint  where the GPU test runs every search form on one finalized group

sequence(seed) is a seeded walk of at most 60 steps that carries the models along, as group_model._Walk does, and records
`result` and `tags` on every Op.  Two root shapes: the narrow one (rows of 256 bytes: several 16-byte units; folded to 7, 6,
5, 3 and 0) and, for every third seed, the wide one (11, 8500, 31, 5), folded to group_model's wide shape (10, 8500, 31, 5).
The orders the walk is written for are tagged for the ledger of tests/test_family_model.py:

  fold_open_tail        a fold of a group whose tail is open at tail % 32 in (1, 7, 8, 31); one insert into the fold and one
                        into the source follow, on the same column, each keeping its own bits below it
  fold_dirty_above      fill, retire everything, set_bits in the retired columns (a retire clears its columns: the planted
                        bits are what the memory keeps), compact (m == 0: nothing launched, the memory kept), a small
                        insert, fold; then both grow over the old memory -- open groups by one-column blocks, each 16 bytes
                        on, finalized ones by inserts: the source shows its old bits, the fold zeros from 16 U on and, in
                        [row_bytes, 16 U), the OR of what the source held there
  fold_planted          set_bits in the pad columns behind an open tail (and in a retired column), a fold, a compaction of
                        the fold with something to close (planted_close) or with nothing to close (planted_nothing)
  fold_empty            a fold of a group of span 0: one that never held a column (never_held), one that a compaction
                        emptied (emptied); inserts and blocks start at column 0 of zero memory
  fold_final, fold_open the fold of a finalized group is finalized (add_columns refused, inserts taken, a checkpoint at
                        once); that of an open group is open, add_columns continues where it would have on the source
  fold_twice            L -> L1 -> L2 next to L -> L2 from one source state
  fold_then_close_src   the source closed right behind the fold, the fold mutated and searched to the end
  copy_from_fold, copy_into_fold
                        lists as copy_model draws them, between a fold and a native group of its parameters
  refuse_*              fold at L2 == L and L2 > L, a copy between a source and its own fold, copy_model's kinds"""
import numpy as np

import copy_model as cm
import group_model as gm
import union_model as um

ERR_ARG, ERR_STATE = gm.ERR_ARG, gm.ERR_STATE
NARROW, WIDE = (8, 2000, 15, 2), (11, 8500, 31, 5)         # (L, capacity, k, num_hash) of the root
MAX_STEPS, MAX_ALIVE = 60, 5
RESIDUES = (1, 7, 8, 31)
COPY_LISTS = ("all", "ascending", "reversed", "shuffled", "one")
REFUSALS = ("fold_same", "fold_longer", "copy_own_fold", "twice", "beyond", "same", "empty", "pad")
ORDERS = ("fold_open_tail", "fold_dirty_above", "fold_planted", "planted_close", "planted_nothing", "fold_empty", "never_held", "emptied",
          "fold_final", "fold_open", "fold_twice", "fold_then_close_src", "copy_from_fold", "copy_into_fold")


def shape_of(seed):
    return WIDE if seed % 3 == 0 else NARROW


def fold_rows(packed, L2):
    """The fold as a plain loop over packed rows: dst[r % 2^L2] |= src[r]."""
    out = np.zeros((1 << L2, packed.shape[1]), dtype=np.uint8)
    for r in range(packed.shape[0]):
        out[r % (1 << L2)] |= packed[r]
    return out


class Family:
    """name -> GroupModel of the groups alive; all share the stride, k and num_hash of `shape`."""

    def __init__(self, shape):
        self.shape, self.stride, self.models = shape, gm.stride_of(shape[1]), {}

    def copy(self):
        f = Family(self.shape)
        f.models = {name: m.copy() for name, m in self.models.items()}
        return f

    def same(self, other):
        return sorted(self.models) == sorted(other.models) and all(m.L == other.models[n].L and m.same(other.models[n]) for n, m in self.models.items())

    def apply(self, op):
        """One Op on the family -> what the call returns: the stats of a fold, a copy's first column, group_model's values,
        or the error code with every model untouched."""
        if op.kind == "new":
            assert op.on not in self.models and len(self.models) < MAX_ALIVE, op
            self.models[op.on] = gm.GroupModel(op.L, self.stride)
            return 0
        if op.kind == "close":
            del self.models[op.on]
            return 0
        if op.kind == "fold":
            r = self.models[op.src].fold(op.L2)
            if isinstance(r, int):
                return r
            assert op.on not in self.models and len(self.models) < MAX_ALIVE, op
            self.models[op.on] = r[0]
            return r[1]
        if op.kind == "copy":
            dst, src = self.models[op.on], self.models[op.src]
            if dst is not src and dst.L != src.L:
                return ERR_ARG
            return cm.copy(dst, src, op.cols)
        if op.kind == "union":
            dst, src = self.models[op.on], self.models[op.src]
            if dst is not src and dst.L != src.L:
                return ERR_ARG
            return um.union(dst, src, op.sets)
        if op.kind == "checkpoint":
            return 0
        return self.models[op.on].apply(op)


class Sequence:
    def __init__(self, seed, shape, ops, queries, fill_query, genomes):
        self.genomes = genomes
        self.seed, self.shape, self.stride, self.ops, self.queries, self.fill_query = seed, shape, gm.stride_of(shape[1]), ops, queries, fill_query
        self.finalizes = any(op.kind == "finalize" for op in ops)
        self.wide = shape == WIDE


class _Walk:
    """The seeded walk: the family is carried along, so that every step is chosen for the state it meets."""

    def __init__(self, seed):
        import kwage_oracle as oracle
        oracle.build()
        self.oracle, self.seed, self.shape = oracle, seed, shape_of(seed)
        self.L, self.cap, self.k, self.nh = self.shape
        self.LF = self.L - 1                                     # the length of the fold that is searched to the end
        self.rng = np.random.default_rng([seed, self.L, self.cap, self.k, self.nh, 1])
        self.fam, self.ops = Family(self.shape), []
        self.folds, self.parent, self.disposable = set(), {}, []
        self.n_inserts = self.n_copies = 0
        rng, k = self.rng, self.k
        # samples as group_model makes them, sized for the fold: their exact filters fill about 0.3 of ITS rows
        glen = k + min(max(int(0.35 * (1 << self.LF) / self.nh), 2), 120) - 1
        self.genomes = [gm.random_dna(rng, glen) for _ in range(6)]
        self._gf = {}
        g = self.genomes
        long1 = gm.random_dna(rng, gm.LONG)
        mut = gm._mutate
        self.queries = [g[0], g[1][1:], g[2][:-1], mut(g[0], [glen - 1]), mut(g[1][1:], [glen - 2]), mut(g[3], [0]),
                        long1, mut(long1, [200, 201, 450]), gm.random_dna(rng, k + 12), gm.random_dna(rng, k + 3), gm.random_dna(rng, k),
                        gm.random_dna(rng, k - 1), g[4][:k + 1] + "N" + g[5]]
        self.fill_query = 6

    # -- helpers
    def m(self, name):
        return self.fam.models[name]

    def genome_filters(self, L):
        if L not in self._gf:
            self._gf[L] = np.stack([self.oracle.bloom_bits_from_sequences([s], self.k, self.nh, L) for s in self.genomes])
        return self._gf[L]

    def emit(self, kind, on, tags=(), **args):
        assert len(self.ops) < MAX_STEPS, (self.seed, kind)
        op = gm.Op(kind, tags, on=on, **args)
        op.result = self.fam.apply(op)
        if kind == "insert" and not op.refused():
            self.n_inserts += 1
            op.tags.add("first%%32=%d" % (op.result % 32))
            if on in self.folds:
                op.tags.add("into_fold")
        if kind == "compact" and op.result[1]["nothing_to_close"]:
            op.tags.add("nothing_to_close")
        self.ops.append(op)
        return op

    def make_room(self, n):
        """Close the oldest groups nobody needs any more until n more fit."""
        while len(self.fam.models) + n > MAX_ALIVE:
            name = self.disposable.pop(0)
            if name in self.fam.models:
                self.emit("close", name)

    def new(self, name, L, tags=()):
        self.make_room(1)
        self.emit("new", name, tags, L=L)

    def fold(self, src, L2, name, tags=()):
        self.make_room(1)
        s = self.m(src)
        op = self.emit("fold", name, list(tags) + ["src_final" if s.finalized else "src_open", "to%d" % L2], src=src, L2=L2)
        assert not op.refused(), (self.seed, op)
        self.folds.add(name)
        self.parent[name] = src
        return op

    def filters(self, L, n, genomes=0):
        """(n filters: random ones at density 1/8 at the root's length, 1/4 below it, the first `genomes` of them exact
        filters of samples; the sample index of each, -1 for a random one)."""
        f = gm.random_filters(self.rng, L, n) & gm.random_filters(self.rng, L, n)
        if L == self.L:
            f &= gm.random_filters(self.rng, L, n)
        ids = [-1] * n
        for i in range(min(n, genomes)):
            f[i], ids[i] = self.genome_filters(L)[i % 6], i % 6
        return f, ids

    def insert(self, on, n, tags=(), genomes=0, reserve=80):
        m = self.m(on)
        n = min(n, m.room() - reserve)
        assert n >= 1, (self.seed, on)
        form = gm.INSERT_FORMS[(self.n_inserts + self.seed) % 3]
        if form == "files" and n > 24:
            form = "host"
        f, ids = self.filters(m.L, n, genomes)
        return self.emit("insert", on, tags, filters=f, form=form, genomes=ids)

    def block(self, on, nf, tags=(), density=0.25):
        m = self.m(on)
        width = (nf + 7) // 8
        image = np.packbits(self.rng.random((m.nrows, 8 * width)) < density, axis=1, bitorder="little")      # (pad bits: garbage)
        return self.emit("add_columns", on, tags, image=image, nf=nf)

    def set_bits(self, on, cols, tags=(), n=6):
        m = self.m(on)
        pick = self.rng.choice(np.asarray(cols, dtype=np.int64), size=n)
        return self.emit("set_bits", on, tags, rows=self.rng.integers(0, m.nrows, size=n), cols=pick)

    def real(self, name):
        return np.flatnonzero(self.m(name).real)

    def checkpoint(self, on, tags=()):
        m, real = self.m(on), self.real(on)
        fs = sorted(int(c) for c in self.rng.choice(real, size=min(3, real.size), replace=False)) if real.size else []
        self.emit("checkpoint", on, list(tags) + (["on_fold"] if on in self.folds else []), fs=fs, search=bool(m.finalized and m.span and real.size))

    def ragged(self, on):
        """An insert after which the tail is open at a column that is no multiple of 8."""
        m = self.m(on)
        first = m.tail_column if m.tail_open else (m.next_byte + 15) // 16 * 128
        n = int(self.rng.integers(9, 16))
        n += (first + n) % 8 == 0
        self.insert(on, n)
        assert m.tail_open and m.tail_column % 8

    def copy(self, dst, src, how):
        """A copy that succeeds: the list drawn as copy_model draws it."""
        real, room = self.real(src), self.m(dst).room()
        assert real.size >= 3 and room > 200, (self.seed, dst, src)
        if how == "all" and real.size > room - 100:
            how = "ascending"
        if how == "all":
            cols = None
        elif how == "one":
            cols = [int(self.rng.choice(real))]
        else:
            n = int(self.rng.integers(2, min(real.size, room - 100, 150) + 1))
            cols = self.rng.choice(real, size=n, replace=False)
            cols = np.sort(cols) if how != "shuffled" else cols
            cols = [int(c) for c in (cols[::-1] if how == "reversed" else cols)]
        tags = ["copy_" + how] + (["copy_from_fold"] if src in self.folds else []) + (["copy_into_fold"] if dst in self.folds else [])
        tags += ["dst_final" if self.m(dst).finalized else "dst_open", "src_final" if self.m(src).finalized else "src_open"]
        op = self.emit("copy", dst, tags, src=src, cols=cols)
        assert not op.refused(), (self.seed, how)
        self.n_copies += 1

    def refuse(self, kind, fold_name, native):
        """One planned refusal; `native` is a native group of fold_name's parameters."""
        mf = self.m(fold_name)
        if kind == "fold_same":
            op = self.emit("fold", "X", ["refuse_fold_same"], src=fold_name, L2=mf.L)
        elif kind == "fold_longer":
            op = self.emit("fold", "X", ["refuse_fold_longer"], src=fold_name, L2=mf.L + 1)
        elif kind == "copy_own_fold":
            child = [c for c, p in self.parent.items() if c in self.fam.models and p in self.fam.models and self.m(p).valid.any()][-1]
            src, dst = (self.parent[child], child) if self.seed % 2 else (child, self.parent[child])
            op = self.emit("copy", dst, ["refuse_copy_own_fold"], src=src, cols=[int(np.flatnonzero(self.m(src).real)[0])])
        else:
            real, dead = self.real(fold_name), np.flatnonzero(~mf.real)
            src, dst = fold_name, native
            if kind == "twice":
                cols = [int(real[0]), int(real[-1]), int(real[0])]
            elif kind == "beyond":
                cols = [int(real[0]), mf.span]
            elif kind == "pad":
                cols = [int(real[0]), int(self.rng.choice(dead))]
            elif kind == "empty":
                cols = []
            else:
                cols, src = [int(self.real(native)[0])], native
            op = self.emit("copy", dst, ["refuse_" + kind], src=src, cols=cols)
        assert op.refused(), (self.seed, kind)

    # -- the orders
    def open_tail(self):
        """fold_open_tail: R's tail steered to a residue, a fold, one insert into the fold and one into R."""
        want = RESIDUES[self.seed % 4]
        r = self.m("R")
        n = (want - r.tail_column) % 32 if r.tail_open else 0
        if not r.tail_open:
            self.insert("R", int(self.rng.integers(2, 20)))
            n = (want - r.tail_column) % 32
        if n:
            self.insert("R", n)
        assert r.tail_open and r.tail_column % 32 == want
        L2 = self.LF if self.shape == WIDE else (7, 6, 5, 3, 0)[self.seed % 5]
        self.fold("R", L2, "T", ["fold_open_tail", "tail%%32=%d" % want])
        a = self.insert("T", int(self.rng.integers(1, 6)), ["after_open_tail"])
        b = self.insert("R", int(self.rng.integers(1, 6)), ["after_open_tail"])
        assert a.result == b.result == r.tail_column - len(b.filters) and a.result % 32 == want
        self.disposable.append("T")

    def main_fold(self):
        """fold_final / fold_open, on half of the seeds fold_then_close_src: the fold F that is searched to the end."""
        r = self.m("R")
        final, close_src = r.finalized, self.seed % 4 in (1, 2)
        self.fold("R", self.LF, "F", ["fold_final" if final else "fold_open"] + (["fold_then_close_src"] if close_src else []))
        if close_src:
            self.emit("close", "R")
        if final:
            self.checkpoint("F", ["after_fold_final"])
            self.block("F", 5, ["refuse_add"])
            assert self.ops[-1].result == ERR_STATE
            self.insert("F", int(self.rng.integers(2, 12)), genomes=2)
        else:
            nf = int(self.rng.integers(13, 40)) | 1
            a = self.block("F", nf, ["block_after_fold_open"])
            if not close_src:
                b = self.block("R", nf, ["block_after_fold_open"], density=0.125)
                assert a.result == b.result

    def copies(self):
        """copy_from_fold and copy_into_fold: F and a native group N of its parameters, three copies."""
        self.new("N", self.LF, ["native_partner"])
        self.insert("N", int(self.rng.integers(5, 30)), genomes=2)
        if self.seed % 4 == 0 and self.finalizing:
            self.emit("finalize", "N")
        pairs = [("N", "F"), ("F", "N"), ("N", "F") if self.seed % 2 else ("F", "N")]
        for i, (dst, src) in enumerate(pairs):
            self.copy(dst, src, COPY_LISTS[(self.seed + 2 * i) % 5])
        self.disposable.append("N")

    def planted(self):
        """fold_planted: bits planted behind F's open tail (and in a retired column), F folded to P, P compacted."""
        f = self.m("F")
        L2 = self.LF - 1 if self.shape == WIDE else (6, 5, 3, 0)[(self.seed // 2) % 4]
        if self.seed % 2 == 0:
            self.emit("compact", "F")
            self.ragged("F")
            self.set_bits("F", np.arange(f.tail_column, f.span), ["set_pad"], n=4)
            self.fold("F", L2, "P", ["fold_planted", "planted_nothing"])
            op = self.emit("compact", "P")
            assert op.result[1]["nothing_to_close"] and self.m("P").matrix[:, self.m("P").tail_column:self.m("P").span].any()
        else:
            self.ragged("F")
            gone = int(self.rng.choice(self.real("F")))
            self.emit("retire", "F", cols=[gone])
            cols = np.array(list(range(f.tail_column, f.span)) + [gone] * 2, dtype=np.int64)
            self.emit("set_bits", "F", ["set_pad", "set_retired"], rows=self.rng.integers(0, f.nrows, size=cols.size), cols=cols)
            self.fold("F", L2, "P", ["fold_planted", "planted_close"])
            assert self.m("P").matrix[:, gone].any() and not self.m("P").valid[gone]
            op = self.emit("compact", "P")
            assert op.result[1]["units"] > 0
        self.insert("P", int(self.rng.integers(2, 20)), ["insert_after_compact"])
        self.disposable.append("P")

    def emptied(self, name, n, finalize=False):
        """A native group at the root's length filled with n columns, all retired, compacted: span 0, the memory kept."""
        self.new(name, self.L)
        self.insert(name, n)
        if finalize:
            self.emit("finalize", name)
        self.emit("retire", name, cols=[int(c) for c in self.real(name)])
        # (a retire clears its columns: what the memory keeps is what set_bits plants in them afterwards)
        cols = np.arange(1, min(self.m(name).span, 256), 3)
        self.emit("set_bits", name, ["set_retired"], rows=self.rng.integers(0, self.m(name).nrows, size=cols.size), cols=cols)
        op = self.emit("compact", name, ["compact_empty"])
        assert op.result[1]["columns"] == 0 and self.m(name).span == 0 and self.m(name).matrix.any()

    def start_at_zero(self, name, how):
        if how == "insert":
            op = self.insert(name, int(self.rng.integers(2, 9)), ["on_empty_fold"])
        else:
            op = self.block(name, int(self.rng.integers(2, 9)), ["on_empty_fold"])
        assert op.result == 0

    def dirty_above(self):
        """fold_dirty_above (and, on every other of these seeds, fold_empty of the emptied group before the small insert)."""
        final = self.seed % 4 == 2
        self.emptied("D", 600, finalize=final)
        if not final:
            self.fold("D", self.LF, "E", ["fold_empty", "emptied"])
            self.start_at_zero("E", "insert")
            self.disposable.append("E")
        self.insert("D", 5)
        self.fold("D", self.LF, "FD", ["fold_dirty_above"])
        d, fd = self.m("D"), self.m("FD")
        for i in range(2):
            if final:                                   # (add_columns is refused: inserts, which own what they grow over)
                self.insert("FD", 70, ["grow_fold"])
                self.insert("D", 70, ["grow_src"])
            else:                                       # a one-column block 16 bytes on: the bytes in between come into sight
                lo = 8 * fd.next_byte
                self.block("FD", 1, ["grow_fold"])
                self.block("D", 1, ["grow_src"], density=0.125)
                hi = 8 * (fd.next_byte - 1)
                assert d.matrix[:, lo:hi].any(), "the source shows its old bits"
                if i == 0:
                    assert np.array_equal(fd.matrix[:, lo:hi], d.matrix[:, lo:hi].reshape(2, fd.nrows, hi - lo).any(axis=0)) and fd.matrix[:, lo:hi].any()
                else:
                    assert not fd.matrix[:, lo:hi].any(), "the fold shows zeros from 16 U on"
        self.disposable += ["FD", "D"]

    def empties(self):
        """fold_empty in both variants: a group that never held a column, and one a compaction emptied."""
        self.new("E0", self.L)
        self.fold("E0", (7, 6, 5, 3, 0)[(self.seed // 2) % 5], "FE", ["fold_empty", "never_held"])
        self.start_at_zero("FE", "insert" if self.seed % 4 == 1 else "block")
        self.disposable += ["E0", "FE"]
        self.emptied("D", 40)
        self.fold("D", self.LF, "E", ["fold_empty", "emptied"])
        self.start_at_zero("E", "block" if self.seed % 4 == 1 else "insert")
        self.disposable += ["D", "E"]

    def twice(self):
        """fold_twice: F -> A -> B next to F -> C."""
        L2 = (5, 3, 0)[(self.seed // 3) % 3]
        self.make_room(3)
        self.fold("F", self.LF - 1, "A", ["fold_twice"])
        self.fold("A", L2, "B", ["fold_twice"])
        self.fold("F", L2, "C", ["fold_twice"]).twin = "B"
        assert self.m("B").same(self.m("C"))
        self.disposable += ["A", "B", "C"]

    # -- the walk
    def run(self):
        rng, seed = self.rng, self.seed
        self.finalizing = seed % 4 != 3
        early = self.finalizing and seed % 2 == 0          # R finalized before it is folded: fold_final; else fold_open
        self.emit("new", "R", L=self.L)
        nf = int(rng.integers(150, 200))
        self.block("R", nf + (nf % 8 == 0), density=0.125)
        self.insert("R", int(rng.integers(8, 30)), genomes=6)
        self.set_bits("R", np.arange(self.m("R").span), ["set_any"])
        self.emit("retire", "R", cols=[int(c) for c in rng.choice(self.real("R")[8:], size=3, replace=False)])
        if early:
            self.emit("finalize", "R")
        self.open_tail()
        self.main_fold()
        if self.finalizing and not early:
            self.emit("finalize", "F")
            if "R" in self.fam.models:
                self.emit("finalize", "R")
        self.copies()
        self.planted()
        for i in range(2):
            self.refuse(REFUSALS[(2 * seed + i) % len(REFUSALS)], "F", "N")
        if self.m("F").finalized:
            self.checkpoint("F")
        if self.shape == NARROW:
            if seed % 3 == 1:
                self.twice()
            if seed % 2 == 0:
                self.dirty_above()
            else:
                self.empties()
        # the end: F closed up, the samples the queries were cut from in again, the last checkpoint
        self.emit("compact", "F")
        self.insert("F", 12, ["insert_after_compact"], genomes=6)
        self.checkpoint("F", ["last"])
        return Sequence(seed, self.shape, self.ops, self.queries, self.fill_query, self.genomes)


def sequence(seed):
    """The steps of a seed: deterministic, host only."""
    return _Walk(seed).run()


def default_seeds(n=12):
    return list(range(n))
