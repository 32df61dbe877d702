"""Two live groups and the copies between them, as a model (no GPU, nothing of the library is imported): A and B are two
group_model.GroupModel's, and a copy is the model's insert of the source model's columns -- the contract of
kwage_group_copy_columns in one line.  sequence(seed) is a seeded walk of at most 40 steps at L = 6 over both groups:
inserts, retires, set_bits (real, dead and pad columns), compactions, one finalize, copies A -> B and B -> A with random
lists (all columns, ascending, reversed, shuffled, a single one), and planned refusals of the copy.  Every step carries
what the model returned when the sequence was made; tests/test_copy_model.py checks the sequences without a device,
tests/test_gpu_copy_model.py replays them on one and compares both groups with the models after every step."""
import numpy as np

import group_model as gm

ERR_ARG = gm.ERR_ARG
L, CAPACITY, K, NH = 6, 2000, 15, 2           # rows of 256 bytes: a copy can cross several 16-byte units
MAX_STEPS = 40


def copy(dst, src, cols):
    """kwage_group_copy_columns on the models -> the first column in dst, or the error code (both models untouched)."""
    if dst is src:
        return ERR_ARG
    if cols is None:
        cols = np.flatnonzero(src.real)
    cols = [int(c) for c in cols]
    if not cols or any(c >= src.span or not src.valid[c] for c in cols) or len(set(cols)) != len(cols):
        return ERR_ARG
    return dst.insert(gm.filters_of(src.matrix[:, cols]))


class _Walk:
    def __init__(self, seed):
        self.seed, self.rng = seed, np.random.default_rng([seed, L, CAPACITY])
        self.m = {name: gm.GroupModel(L, gm.stride_of(CAPACITY)) for name in "AB"}
        self.ops = []

    def emit(self, kind, on, tags=(), **args):
        op = gm.Op(kind, tags, on=on, **args)
        if kind == "copy":
            op.result = copy(self.m[on], self.m[op.src], op.cols)
        else:
            op.result = self.m[on].apply(op)
        self.ops.append(op)
        return op

    def room(self, name):
        m = self.m[name]
        return 8 * m.stride - (m.tail_column if m.tail_open else (m.next_byte + 15) // 16 * 16 * 8)

    def insert(self, on, n):
        n = min(n, self.room(on) - 200)
        if n >= 1:
            f = gm.random_filters(self.rng, L, n) & gm.random_filters(self.rng, L, n)
            self.emit("insert", on, filters=f)

    def real(self, name):
        return np.flatnonzero(self.m[name].real)

    def copy(self, dst, src):
        """A copy that succeeds: the list drawn for the state both groups are in."""
        if self.real(src).size < 3:
            self.insert(src, int(self.rng.integers(3, 20)))
        real, room = self.real(src), self.room(dst)
        how = ("all", "ascending", "reversed", "shuffled", "one")[int(self.rng.integers(5))]
        if how == "all" and real.size > room - 100:
            how = "ascending"
        if how == "all":
            cols = None
        elif how == "one":
            cols = [int(self.rng.choice(real))]
        else:
            n = int(self.rng.integers(2, min(real.size, max(room - 100, 2), 150) + 1))
            cols = self.rng.choice(real, size=n, replace=False)
            cols = np.sort(cols) if how != "shuffled" else cols
            cols = [int(c) for c in (cols[::-1] if how == "reversed" else cols)]
        op = self.emit("copy", dst, ["copy_" + how, src + dst], src=src, cols=cols)
        assert not op.refused(), (self.seed, how)

    def refuse_copy(self, dst, src, i):
        ms, real, dead = self.m[src], self.real(src), np.flatnonzero(~self.m[src].real)
        kinds = ["twice", "beyond", "same", "empty"] + (["pad"] if dead.size else [])
        kind = kinds[(self.seed + i) % len(kinds)]
        if real.size < 2:
            kind = "beyond"
        if kind == "twice":
            cols = [int(real[0]), int(real[-1]), int(real[0])]
        elif kind == "beyond":
            cols = [int(real[0]) if real.size else 0, ms.span]
        elif kind == "pad":
            cols = [int(real[0]), int(self.rng.choice(dead))]
        elif kind == "empty":
            cols = []
        else:
            cols, src = [int(real[0])], dst
        op = self.emit("copy", dst, ["refuse_" + kind], src=src, cols=cols)
        assert op.refused(), (self.seed, kind)

    def retire(self, on):
        real = self.real(on)
        if real.size >= 6:
            how = int(self.rng.integers(3))
            cols = [int(real[-1])] if how == 0 else [int(c) for c in self.rng.choice(real, size=int(self.rng.integers(1, 5)), replace=False)]
            self.emit("retire", on, cols=cols)

    def set_bits(self, on):
        m = self.m[on]
        if m.span:
            n = 6
            self.emit("set_bits", on, rows=self.rng.integers(0, m.nrows, size=n), cols=self.rng.integers(0, m.span, size=n))

    def run(self):
        rng = self.rng
        # the beginning: a file-like block in A (ragged: pad columns behind it), a first insert in B
        nf = int(rng.integers(100, 200)) | 1
        image = np.packbits(rng.random((1 << L, 8 * ((nf + 7) // 8))) < 0.25, axis=1, bitorder="little")
        self.emit("add_columns", "A", image=image, nf=nf)
        self.insert("B", int(rng.integers(5, 60)))
        deck = ["copyAB"] * 4 + ["copyBA"] * 4 + ["insert"] * 4 + ["retire"] * 5 + ["set_bits"] * 4 + ["compact"] * 3 + ["finalize"] + ["refuse"] * 2
        rng.shuffle(deck)
        refusals = 0
        for item in deck:
            on = "AB"[int(rng.integers(2))]
            if len(self.ops) >= MAX_STEPS - 2 and not item.startswith("copy"):
                continue                                   # (a copy may take an insert before it: the copies come first)
            if item == "copyAB":
                self.copy("B", "A")
            elif item == "copyBA":
                self.copy("A", "B")
            elif item == "insert":
                self.insert(on, int(rng.integers(1, 40)))
            elif item == "retire":
                self.retire(on)
            elif item == "set_bits":
                self.set_bits(on)
            elif item == "compact":
                self.emit("compact", on)
            elif item == "finalize":
                self.emit("finalize", on)
            else:
                self.refuse_copy(on, "AB"["BA".index(on)], refusals)
                refusals += 1
        return self.ops


def sequence(seed):
    """The steps of a seed: deterministic, host only."""
    return _Walk(seed).run()


def apply(models, op):
    """One step on the models {"A": .., "B": ..} -> what the call returns."""
    if op.kind == "copy":
        return copy(models[op.on], models[op.src], op.cols)
    return models[op.on].apply(op)


def fresh_models():
    return {name: gm.GroupModel(L, gm.stride_of(CAPACITY)) for name in "AB"}


SEEDS = list(range(8))
