"""Walks with the union of columns (no GPU, nothing of the library is imported): family_model's family of live groups
under group_model's mutators, the fold and union_model.union (`union`: on = destination, src = source, sets = member lists),
so that every union meets the state earlier calls left -- memory a compaction kept, units an earlier union stored, folds,
open tails -- and every group alive is compared after every step (tests/test_gpu_union_walk.py replays them on the device,
tests/test_union_walk.py checks them without one).

sequence(seed) is a seeded walk of at most 60 steps and at most five groups alive; every third seed walks on
family_model.WIDE, the others on NARROW.  Member lists are union_model.lists_of's, drawn from the source model's state at
that step; filters are family_model._Walk.filters' (density 1/8 at the root, 1/4 below it).  The orders, tagged for the
ledger:

  union_same_open_tail  the tail steered to tail % 128 in (1, 31, 33, 127), one same-group union (it lands at the next
                        multiple of 128), one insert right behind the union and, on an open group, one block at the
                        16-byte boundary behind that
  union_over_dirty      a native group filled, everything retired, set_bits in the retired columns, compacted (m == 0: the
                        memory kept), a few columns inserted, a same-group union: the columns skipped, from the end of the
                        insert's last word to the landing, hold set bits and are not valid.  An open group then grows by
                        one-column blocks (union_model.reveal_ops) until the dirty bytes above the union's last 32-bit word
                        are in sight, a finalized one goes straight to a checkpoint; then a compaction with something to
                        close, an insert, a checkpoint
  union_of_unions       a union U1, then a same-group union whose sets mix U1's columns with original ones: every
                        second-level column is the flat union of the originals underneath
  union_merge           a union, all its members retired, a compaction, an insert (the six samples' filters), a checkpoint
  union_into_fold, union_from_fold, union_within_fold
                        F (the fold of R at LF) and a native partner N of F's parameters; on the narrow seeds also a fold
                        at L2 in (5, 3, 0) that receives a same-group union
  union_fold_commutes   from one state of R, whose tail is open: union then fold to L2 next to fold to L2 then the same
                        union -- the same model (op.twin names the other group); the pad gap is folded too
  union_final, union_open
                        the destination is finalized (a checkpoint at once, add_columns refused) or open (add_columns goes
                        on behind), each within one group and between two
  union_above_kib       wide seeds: a native group at the root's parameters filled until its next landing is 8064, a union
                        of 200 sets across column 8192, finalize, a checkpoint whose fs columns lie on both sides of 8192
  union_full_row        a union of exactly 8 * stride - landing sets: the span is the row, room 0; one more set is refused
  refuse_*              own_fold (a source and its own fold, both directions over the seeds), retired, pad (a column an
                        earlier same-group union skipped: below the span, never valid), beyond (the span itself),
                        empty_set, no_sets, capacity -- each with every model untouched

Among the samples' filters every walk makes one union of exactly the samples queries 1 and 2 were cut from (`genome_union`);
the last query is the first half of the one, an N, and the first half of the other."""
import numpy as np

import family_model as fm
import group_model as gm
import union_model as um

ERR_ARG, ERR_STATE = gm.ERR_ARG, gm.ERR_STATE
MAX_STEPS, MAX_ALIVE = fm.MAX_STEPS, fm.MAX_ALIVE
RESIDUES = (1, 31, 33, 127)
LISTS = um.LISTS
REFUSALS = ("own_fold", "retired", "pad", "beyond", "empty_set", "no_sets", "capacity")
ORDERS = ("union_same_open_tail", "union_over_dirty", "union_of_unions", "union_merge", "union_into_fold", "union_from_fold",
          "union_within_fold", "union_fold_commutes", "union_final", "union_open", "union_above_kib", "union_full_row")
SETS = {"one": 1, "all": 1, "129sets": 129, "dwords": 5, "repeat": 2, "200sets": 200, "unequal": 7}


def shape_of(seed):
    return fm.shape_of(seed)


def landing(m, same):
    """Where a union into model m lands: the open tail between two groups, the next multiple of 128 at or above the span
    within one."""
    return m.tail_column if m.tail_open and not same else (m.next_byte + 15) // 16 * 128


class _Walk(fm._Walk):
    def __init__(self, seed):
        super().__init__(seed)
        self.rng = np.random.default_rng([seed, self.L, self.cap, self.k, self.nh, 2])
        g, h = self.genomes, len(self.genomes[0]) // 2
        assert h >= self.k
        self.queries = self.queries + [g[1][:h] + "N" + g[2][:h]]
        self.pad = {}                                         # group -> a column a same-group union skipped

    # -- helpers
    def emit(self, kind, on, tags=(), **args):
        if kind == "union":
            d, same = self.m(on), args["src"] == on
            tags = list(tags) + ["same_group" if same else "two_group", "dst_final" if d.finalized else "dst_open"]
            tags += ["src_fold"] if args["src"] in self.folds else []
            tags += ["dst_fold"] if on in self.folds else []
        return super().emit(kind, on, tags, **args)

    def checkpoint(self, on, tags=(), fs=None):
        m, real = self.m(on), self.real(on)
        if fs is None:
            fs = sorted(int(c) for c in self.rng.choice(real, size=min(3, real.size), replace=False)) if real.size else []
        self.emit("checkpoint", on, list(tags) + (["on_fold"] if on in self.folds else []), fs=sorted(fs), search=bool(m.finalized and m.span and real.size))

    def union(self, dst, src, kind, tags=(), reserve=0):
        """A union that succeeds: the lists of `kind` from src's state (a smaller kind where the row has no room)."""
        same = dst == src
        room = 8 * self.m(dst).stride - landing(self.m(dst), same)
        if SETS[kind] + reserve > room:
            kind = "unequal"
        assert SETS[kind] + reserve <= room, (self.seed, dst, src, kind, room)
        sets = um.lists_of(self.rng, kind, self.m(src))
        want = landing(self.m(dst), same)
        op = self.emit("union", dst, list(tags) + ["list_" + kind], src=src, sets=sets)
        assert op.result == want, (self.seed, op, op.result, want)
        return op

    def refused_block(self, on):
        self.block(on, 5, ["refuse_add"])
        assert self.ops[-1].result == ERR_STATE

    def final_or_open(self, on, first):
        """union_final / union_open behind a union whose first column is `first`."""
        op = self.ops[-1]
        if self.m(on).finalized:
            op.tags.add("union_final")
            self.checkpoint(on, ["after_union_final"], fs=[first, int(self.real(on)[0])])
            self.refused_block(on)
        else:
            op.tags.add("union_open")
            b = self.block(on, int(self.rng.integers(3, 12)), ["block_after_union_open"])
            assert b.result == (self.m(on).next_byte - (b.nf + 7) // 8) * 8 and b.result >= first + len(op.sets)

    # -- the orders
    def same_open_tail(self):
        want = RESIDUES[(self.seed + self.seed // 4) % 4]
        r = self.m("R")
        assert r.tail_open
        n = (want - r.tail_column) % 128
        if n:
            self.insert("R", n)
        assert r.tail_open and r.tail_column % 128 == want
        tail, word_end = r.tail_column, (r.tail_column + 31) // 32 * 32
        op = self.union("R", "R", LISTS[self.seed % 7], ["union_same_open_tail", "tail%%128=%d" % want], reserve=600)
        assert op.result == (tail + 127) // 128 * 128 > tail and not r.valid[tail:op.result].any() and not r.matrix[:, tail:word_end].any()
        self.pad["R"] = int(self.rng.integers(tail, op.result))
        a = self.insert("R", int(self.rng.integers(1, 6)), ["behind_union"])
        assert a.result == op.result + len(op.sets)
        if not r.finalized:
            b = self.block("R", int(self.rng.integers(3, 20)), ["behind_union"], density=0.125)
            assert b.result == (a.result + len(a.filters) + 127) // 128 * 128

    def of_unions(self):
        r, rng = self.m("R"), self.rng
        real = self.real("R")
        first = [[int(c) for c in rng.choice(real, size=int(rng.integers(2, 4)), replace=False)] for _ in range(6)]
        u1 = self.emit("union", "R", ["union_of_unions", "level1"], src="R", sets=first).result
        assert u1 >= 0
        second, flat = [], []
        for j in range(5):
            a, b = (int(x) for x in rng.choice(6, size=2, replace=False))
            c = int(rng.choice(real))
            second.append([u1 + a, c, u1 + b])
            flat.append(first[a] + [c] + first[b])
        second += [[u1 + 5], [u1 + j for j in range(6)]]
        flat += [first[5], [c for s in first for c in s]]
        u2 = self.emit("union", "R", ["union_of_unions", "level2"], src="R", sets=second).result
        assert u2 == (u1 + 6 + 127) // 128 * 128
        for j, cols in enumerate(flat):
            assert np.array_equal(r.matrix[:, u2 + j], r.matrix[:, cols].any(axis=1)) and r.matrix[:, u2 + j].any()
        self.final_or_open("R", u2)

    def fold_unions(self):
        """F = fold of R at LF, N native at F's parameters: into, out of and within the fold; own_fold refused."""
        seed = self.seed
        self.fold("R", self.LF, "F", ["main_fold"])
        self.new("N", self.LF, ["native_partner"])
        self.insert("N", int(self.rng.integers(70, 100)), genomes=2)
        if self.finalizing and seed % 4 == 0:
            self.emit("finalize", "N")
        op = self.union("F", "N", LISTS[(seed + 2) % 7], ["union_into_fold"], reserve=500)
        self.final_or_open("F", op.result)
        self.union("N", "F", LISTS[(seed + 4) % 7], ["union_from_fold"], reserve=300)
        f = self.m("F")
        tail = f.tail_column if f.tail_open else None
        op = self.union("F", "F", LISTS[(seed + 5) % 7], ["union_within_fold", "to%d" % self.LF], reserve=250)
        if tail is not None and op.result > tail:
            self.pad["F"] = int(self.rng.integers(tail, op.result))
        src, dst = ("R", "F") if seed % 2 else ("F", "R")
        op = self.emit("union", dst, ["refuse_own_fold"], src=src, sets=[[int(self.real(src)[0])]])
        assert op.refused()

    def refuse(self, kind):
        """One planned refusal with F as the source, within F or into N."""
        f = self.m("F")
        dst = "N" if self.seed % 2 else "F"
        real = self.real("F")
        if kind == "retired":
            gone = [c for c in self.retired if not f.valid[c]]
            sets = [[int(real[0])], [int(real[1]), int(gone[0])]]
        elif kind == "pad":
            c = self.pad.get("F", self.pad["R"])
            assert c < f.span and not f.valid[c]
            sets = [[int(real[0]), c]]
        elif kind == "beyond":
            sets = [[int(real[0])], [f.span]]
        elif kind == "empty_set":
            sets = [[int(real[0])], [], [int(real[1])]]
        else:
            assert kind == "no_sets"
            sets = []
        op = self.emit("union", dst, ["refuse_" + kind], src="F", sets=sets)
        assert op.refused(), (self.seed, kind)

    def commutes(self):
        """union_fold_commutes: R -> Y (fold), union on R, R -> Z (fold), the same union on Y: Y is Z."""
        r = self.m("R")
        if not (r.tail_open and r.tail_column % 128):
            self.ragged("R")
        assert r.tail_open and r.tail_column % 128
        L2 = self.LF - 1 if self.shape == fm.WIDE else (5, 3, 0)[(self.seed // 3) % 3]
        self.make_room(2)
        self.fold("R", L2, "Y", ["union_fold_commutes"])
        u = self.union("R", "R", LISTS[(self.seed + 1) % 7], ["union_fold_commutes"], reserve=0)
        self.fold("R", L2, "Z", ["union_fold_commutes"])
        op = self.emit("union", "Y", ["union_fold_commutes", "union_within_fold", "to%d" % L2], src="Y", sets=u.sets)
        op.twin = "Z"
        assert op.result == u.result and self.m("Y").same(self.m("Z")) and self.m("Y").L == self.m("Z").L == L2
        self.disposable += ["Y", "Z"]

    def over_dirty(self, final):
        rng = self.rng
        self.new("D", self.L)
        self.insert("D", 700)
        if final:
            self.emit("finalize", "D")
        d = self.m("D")
        self.emit("retire", "D", cols=[int(c) for c in self.real("D")])
        cols = np.arange(1, d.span, 2)
        self.emit("set_bits", "D", ["set_retired"], rows=rng.integers(0, d.nrows, size=cols.size), cols=cols)
        op = self.emit("compact", "D", ["compact_empty"])
        assert op.result[1]["columns"] == 0 and d.span == 0 and d.matrix.any()
        a = self.insert("D", 6)
        assert a.result == 0
        word_end = 32
        u = self.union("D", "D", ("one", "repeat", "unequal")[(self.seed // 3) % 3], ["union_over_dirty"])
        n = len(u.sets)
        assert u.result == 128 and d.matrix[:, word_end:128].any() and not d.valid[word_end:128].any() and not d.matrix[:, 6:word_end].any()
        last_word = ((u.result + n - 1) // 32 + 1) * 32
        assert last_word % 128 and d.matrix[:, last_word:256].any()           # dirty bits in the union's own last unit
        if final:
            self.checkpoint("D", ["dirty_below_span"], fs=[u.result, 0])
        else:
            for b in um.reveal_ops(d, "D"):
                self.emit("add_columns", "D", ["reveal"], image=b.image, nf=b.nf)
                if d.span > 256:
                    break
            assert d.matrix[:, last_word:d.span - 8].any() and not d.valid[last_word:d.span - 8].any()
        op = self.emit("compact", "D", ["compact_dirty"])
        assert op.result[1]["units"] > 0
        self.insert("D", int(rng.integers(2, 20)), ["insert_after_compact"])
        self.checkpoint("D", ["after_dirty"])
        self.disposable.append("D")

    def above_kib(self):
        self.new("K", self.L)
        self.insert("K", 8064)
        k = self.m("K")
        assert landing(k, True) == 8064 == k.tail_column
        u = self.union("K", "K", "200sets", ["union_above_kib"])
        assert u.result == 8064 and k.span > 8192
        if self.finalizing:
            self.emit("finalize", "K")
        self.checkpoint("K", ["above_kib"], fs=[8100, 8191, 8192, 8263])
        if self.finalizing:
            self.emit("close", "K")                   # (searched; the widest matrix of the walk is not read again after every later step)
        else:
            self.disposable.append("K")               # (not searched: its columns go through a file and back at the end)

    def full_row(self, on, src):
        m = self.m(on)
        n = 8 * m.stride - landing(m, on == src)
        assert n >= 1
        real = self.real(src)
        sets = [[int(c)] for c in self.rng.choice(real, size=n)]
        op = self.emit("union", on, ["union_full_row", "list_full"], src=src, sets=sets)
        assert not op.refused() and m.span == 8 * m.stride and m.room() == 0
        op = self.emit("union", on, ["refuse_capacity"], src=src, sets=[[int(real[0])]])
        assert op.refused()

    def merge_and_end(self):
        """union_merge on F, the genome union, the last checkpoint."""
        rng, f = self.rng, self.m("F")
        real = self.real("F")
        members = [int(c) for c in rng.choice(real, size=min(12, real.size), replace=False)]
        sets = [members[:5], members[5:9], members[9:], [members[0], members[-1]]]
        u = self.emit("union", "F", ["union_merge"], src="F", sets=[s for s in sets if s])
        assert not u.refused()
        self.emit("retire", "F", cols=members)
        op = self.emit("compact", "F")
        assert op.result[1]["units"] > 0
        a = self.insert("F", 12, ["insert_after_compact"], genomes=6)
        self.checkpoint("F", ["after_merge"])
        g1, g2 = a.result + 1, a.result + 2
        more = [[int(c) for c in rng.choice(self.real("F"), size=2, replace=False)] for _ in range(3)]
        u = self.emit("union", "F", ["genome_union"], src="F", sets=[[g1, g2]] + more + [[g2, g1, a.result + 3]])
        assert not u.refused()
        self.checkpoint("F", ["last"], fs=[u.result, g1, g2])

    # -- the walk
    def run(self):
        rng, seed = self.rng, self.seed
        narrow = self.shape == fm.NARROW
        self.finalizing = seed % 4 != 3
        early = self.finalizing and seed % 2 == 0
        self.emit("new", "R", L=self.L)
        nf = int(rng.integers(150, 200))
        self.block("R", nf + (nf % 8 == 0), density=0.125)
        self.insert("R", int(rng.integers(8, 30)), genomes=6)
        self.retired = [int(c) for c in rng.choice(self.real("R")[8:], size=3, replace=False)]
        self.emit("retire", "R", cols=self.retired)
        if early:
            self.emit("finalize", "R")
        self.same_open_tail()
        self.of_unions()
        self.fold_unions()
        if self.finalizing and not early:
            self.emit("finalize", "F")
            self.emit("finalize", "R")
        kinds = REFUSALS[1:6]
        for i in range(2):
            self.refuse(kinds[(2 * seed + i) % 5])
        if seed % 3 == 2 or seed == 9:
            if seed % 2:
                self.full_row("N", "N")
            else:
                self.full_row("N", "F")
        self.disposable.append("N")
        self.commutes()
        self.disposable.append("R")
        if narrow and seed % 3 == 1:
            self.over_dirty(final=self.finalizing and seed % 2 == 0)
        if not narrow:
            self.above_kib()
        self.merge_and_end()
        return fm.Sequence(seed, self.shape, self.ops, self.queries, self.fill_query, self.genomes)


def sequence(seed):
    """The steps of a seed: deterministic, host only."""
    return _Walk(seed).run()


def default_seeds(n=12):
    return list(range(n))
