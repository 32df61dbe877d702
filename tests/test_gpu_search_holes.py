"""kwage_search at its gather-kernel instantiations a second time, on groups with DEAD columns, against the CPU oracle.

Every gather kernel runs over the whole row stride and applies the group's valid mask itself; the groups of
test_gpu_search_shapes.py are one block without a hole, so there the mask only ever cuts the row's end.  Here every group
is that same image with the columns of search_holes.dead_columns retired -- single columns of the first unit, a whole
16-byte unit, every other column of a unit, a whole 128-byte column group, both sides of every KiB-step boundary, a whole
KiB-step, the row's tail -- and with set bits put back into search_holes.hot_columns of them, in every row of every
planted query: a kernel that takes a dead column for a live one reports it for every planted query at every threshold.

The cases are search_holes.HOLE_CASES; groups, batches and the run of a case are search_groups.py's.  The expected list is
the unholed group's oracle list without the records of dead columns: it must be non-empty and shorter than the unholed
one.  Each case asserts the exact name it reports, every query's k-mer count, the whole hit list, that no record names a
dead column, and zeroed exchange buffers after every persistent or early-exit form; each test checks at its end that it
reached all the instantiations the ledger (test_search_holes_ledger.py) assigns to its family.  Presence, top-k and score
searches on two of the groups derive their references from the same list.  Every comparison is exact.
KWAGE_SEARCH_FULL_GRID=1 adds the threshold sweep and the knob variants of the unholed file."""
import numpy as np
import pytest

import search_holes as sh
import search_shapes as ss
from search_groups import GROUP_BATCHES, Env, Group, run_family
from topk_reference import assert_hits_equal

pytestmark = pytest.mark.gpu

TOPK_MAX = 1024          # include/kwage_amd.h KWAGE_TOPK_MAX: the largest k kwage_search_topk takes


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def env(ka, oracle):
    e = Env(ka, oracle, group=HoledGroup)
    yield e
    e.close()


def bytes_of(columns, nb):
    """uint8 [nb]: the listed columns as set bits of a row."""
    bits = np.zeros(8 * nb, dtype=bool)
    bits[columns] = True
    return np.packbits(bits, bitorder="little")


class HoledGroup(Group):
    """The unholed group's image, its dead columns retired, set bits put back into the hot ones, finalized; the built state
    is checked against the host model before anything is searched."""

    def load(self, env, img):
        g, W, nrows = self.g, self.W, 1 << self.L
        nb = (W + 7) // 8
        dead, hot = sh.dead_columns(W), sh.hot_columns(W)
        if self.key[0] == "count_dense":
            hot_rows = np.arange(nrows)
        else:
            hot_rows = np.unique(np.concatenate([env.rows(s, self.L)[:, :self.nh].reshape(-1)
                                                 for bk in GROUP_BATCHES[self.key[0]] for s in env.batch(bk).plant]))
        g.add_columns(img, W)
        g.retire_columns(dead)
        g.set_bits(np.repeat(hot_rows, hot.size), np.tile(hot, hot_rows.size))
        g.finalize()
        self.real = sh.real_columns(W, g.column_span)
        assert g.num_columns == W - dead.size and np.array_equal(g.real_columns(), self.real), self.key
        # the pattern kills planted columns and leaves their neighbours in the same byte alive
        per = ~np.concatenate([self.real[:W], np.zeros(8 * nb - W, dtype=bool)]).reshape(nb, 8)[self.spots]
        assert per.all(axis=1).any() and (per.any(axis=1) & ~per.all(axis=1)).any(), self.key
        # a few dozen rows against the model: dead columns read zero, hot ones carry their bits, the rest is the image
        rng = np.random.default_rng(W)
        sample = np.unique(np.concatenate([[0, nrows - 1], rng.choice(hot_rows, size=min(24, hot_rows.size), replace=False),
                                           rng.integers(0, nrows, size=24)])).astype(np.int64)
        model = img[sample, :nb] & ~bytes_of(dead, nb)
        model[np.isin(sample, hot_rows)] |= bytes_of(hot, nb)
        got = g.read_rows(sample)
        assert got.shape[1] >= nb and np.array_equal(got[:, :nb], model), (self.key, np.argwhere(got[:, :nb] != model)[:5])
        assert np.isin(sample, hot_rows).any() and (model & bytes_of(hot, nb)).any()
        self.sample, self.model = sample, model

    def expected(self, env, batch, t):
        key = ("holes", self.key, batch.key, t)
        if key not in env.expected:
            full = Group.expected(self, env, batch, t)
            exp = full[self.real[full["column"]]]
            # the reference alone: something is left to find, and the oracle reported a column that is dead now
            assert 0 < exp.size < full.size, (key, exp.size, full.size)
            env.expected[key] = exp
        return env.expected[key]

    def check_hits(self, hits, what):
        cols = hits["column"].astype(np.int64)
        bad = (cols >= self.real.size) | ~self.real[np.minimum(cols, self.real.size - 1)]
        assert not bad.any(), ("a record of a dead column", what, hits[bad][:5])


def test_and_narrow(env):
    run_family(env, sh.HOLE_CASES, "and_narrow")


def test_and_screen_then_refine(env):
    run_family(env, sh.HOLE_CASES, "and_screen")


def test_and_walk(env):
    run_family(env, sh.HOLE_CASES, "and_walk")


def test_and_band_walk(env):
    run_family(env, sh.HOLE_CASES, "and_band_walk")


def test_and_kernel(env):
    run_family(env, sh.HOLE_CASES, "and_kernel")


def test_count_screen_then_refine(env):
    run_family(env, sh.HOLE_CASES, "count_screen")


def test_count_walk_truncated_then_refine(env):
    run_family(env, sh.HOLE_CASES, "count_walk_trunc")


def test_count_walk(env):
    run_family(env, sh.HOLE_CASES, "count_walk_pf")


def test_count_kernel(env):
    run_family(env, sh.HOLE_CASES, "count_kernel")


def test_count_segments_and_combine(env):
    run_family(env, sh.HOLE_CASES, "count_segments")


def test_count_narrow(env):
    run_family(env, sh.HOLE_CASES, "count_narrow")


@pytest.mark.parametrize("key,bk,t", sh.OTHER_FORMS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_other_search_forms(env, key, bk, t):
    """Presence, top-k and dense scores: their references all come from the masked list of the threshold search."""
    g, b = env.group(key), env.batch(bk)
    exp = g.expected(env, b, t)
    span = g.g.column_span
    want = np.zeros((len(b.seqs), span), dtype=bool)
    want[exp["query"], exp["column"]] = True
    p = g.g.search_presence(b.b, t)
    assert np.array_equal(p.num_query_kmer, b.nkmer) and np.array_equal(p.passing, want.sum(axis=1))
    got = p.unpack()
    assert not got[:, span:].any() and np.array_equal(got[:, :span], want), np.argwhere(got[:, :span] != want)[:5]
    # top-k with the threshold as its floor: the same list, every query's cut at the k best (score descending, column
    # ascending) -- 1024 is the largest k the search takes
    order = np.lexsort((exp["column"], -exp["num_match"].astype(np.int64), exp["query"]))
    rank = np.arange(exp.size) - np.searchsorted(exp["query"][order], exp["query"][order], side="left")
    top = np.sort(order[rank < TOPK_MAX])
    r = g.g.search_topk(b.b, TOPK_MAX, t)
    g.check_hits(r.hits, "top-k")
    assert_hits_equal(r.hits, exp[top], "top-k %s" % (key,))
    s = g.g.search_scores(b.b)
    assert s.scores.shape == (len(b.seqs), span) and not s.scores[:, ~g.real].any(), np.argwhere(s.scores[:, ~g.real])[:5]
    assert np.array_equal(s.scores[exp["query"], exp["column"]], exp["num_match"])
    assert np.array_equal(s.num_query_kmer, b.nkmer)


def test_compaction_with_hot_dead_columns(env):
    """A group of its own: compacting it moves every survivor below the dead columns' set bits and must leave none behind."""
    case = [c for c in sh.HOLE_CASES if c.test == "and_walk" and c.group == ("and", 5)][0]
    assert case.name == "and_walk_kernel<5,4>" and case.knobs == ss.WALK
    b = env.batch(case.batch)
    g = HoledGroup(env, case.group)
    try:
        def walk():
            with env.ctx.tuning(**case.knobs):
                r = g.g.search(b.b, case.t, 0)
            assert r.search_kernel == case.name and np.array_equal(r.num_query_kmer, b.nkmer), r.search_kernel
            left = env.ctx.scratch_nonzero()
            assert not any(left.values()), left
            return r.hits
        before = walk()
        g.check_hits(before, "before")
        assert_hits_equal(before, g.expected(env, b, case.t), "before")
        real, stride, span = g.real, g.g.row_stride, g.g.column_span
        new, st = g.g.compact()
        m = int(real.sum())
        assert st["columns"] == m == g.g.num_columns and st["span_before"] == span and g.g.column_span == (m + 7) // 8 * 8
        assert np.array_equal(new, np.where(real, np.cumsum(real) - 1, -1))
        assert g.g.row_stride == stride                     # (the same stride: the same kernel)
        after = walk()
        want = before.copy()
        want["column"] = new[before["column"]]
        assert (after["column"] < m).all(), after[after["column"] >= m][:5]
        assert_hits_equal(after, want, "after")
        # the survivors' bits, in their order; the pad bits behind column m - 1 are zero
        bits = np.unpackbits(g.model, axis=1, bitorder="little")[:, :g.W][:, real[:g.W]]
        assert np.array_equal(g.g.read_rows(g.sample), np.packbits(bits, axis=1, bitorder="little"))
        assert np.array_equal(g.g.real_columns(), np.arange(g.g.column_span) < m)
    finally:
        g.g.close()
