"""kwage_search at every gather-kernel instantiation of engine.hip, against the CPU oracle.

The cases are the table of search_shapes.py (CASES): each one asserts the exact name it reports, compares the whole hit
list (query, column, num_match in (query, column) order) and every query's k-mer count with the oracle's, and each test
checks at its end that it reached all the instantiations of its family.  After every persistent or early-exit form the
exchange buffers must read zero again.

Wide groups stay cheap for the oracle: a group is made of copies of a narrow base block.  Byte j of every row is base byte
map[j], drawn at random (not periodic in 128 or 1024 columns), so column j is base column 8 map[j] + j % 8; a few base
bytes are used once only, at the first, middle and last 128-byte group and at KiB-step boundaries, and hold the planted
columns: every row of a query (count n), the rows of its first thr and thr - 1 distinct k-mers, none (count 0), and at
t = 1 all but one row of one k-mer.  The oracle counts the base; the map spreads its lists over the group.  Pad bits hold
garbage.  KWAGE_SEARCH_FULL_GRID=1 adds the threshold sweep and the list-capacity and unit-length knob variants."""
import os

import numpy as np
import pytest

import search_shapes as ss
from topk_reference import HIT_DTYPE, assert_hits_equal, pack_columns, rand_bits

pytestmark = pytest.mark.gpu

FULL_GRID = os.environ.get("KWAGE_SEARCH_FULL_GRID", "0") == "1"
SWEEP = (1.0, 0.9, 0.8, 0.5, 0.05)
K = ss.K
PERSISTENT = ("walk", "screen", "trunc", "refine")


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def env(ka, oracle):
    e = Env(ka, oracle)
    yield e
    e.close()


class Env:
    """The module's context, groups and batches, built on first use and shared by the tests."""

    def __init__(self, ka, oracle):
        self.ka, self.oracle = ka, oracle
        self.ctx = ka.Context(0)
        self.ncu = int(self.ctx.fingerprint()["cus"])
        self.groups, self.batches, self.expected = {}, {}, {}
        self.rows_cache = {}

    def close(self):
        for g in self.groups.values():
            g.g.close()
        for b in self.batches.values():
            b.b.close()
        self.ctx.close()

    # ---- batches --------------------------------------------------------------------------------------------------------
    def batch(self, key):
        if key not in self.batches:
            self.batches[key] = Batch(self, key)
        return self.batches[key]

    # ---- groups ---------------------------------------------------------------------------------------------------------
    def group(self, key):
        if key not in self.groups:
            self.groups[key] = Group(self, key)
        return self.groups[key]

    def rows(self, seq, L):
        """[distinct k-mers, 5] row indices of seq's sorted distinct k-mers (hash h's rows do not depend on num_hash)."""
        if (seq, L) not in self.rows_cache:
            km = self.oracle.unique_kmers(seq, K)
            self.rows_cache[(seq, L)] = self.oracle.row_indices(km, K, 5, L)
        return self.rows_cache[(seq, L)]


class Batch:
    def __init__(self, env, key):
        seqs, plant = ss.batch_seqs(key, env.ncu)
        self.key, self.seqs, self.plant = key, seqs, [seqs[i] for i in plant]
        self.b = env.ka.Batch(env.ctx, seqs)
        self.distinct = list(dict.fromkeys(seqs))
        n = {s: len(env.oracle.unique_kmers(s, K)) for s in self.distinct}
        self.nkmer = np.array([n[s] for s in seqs], dtype=np.uint32)


GROUP_BATCHES = {"and": ("and",), "and_wide": ("and_wide",), "and_narrow": ("and_short",), "count": ("c7", "c10", "c14a", "c14b", "c20a", "c20b", "c32r"),
                 "count_narrow": ("n7", "n10", "n14"), "count_dense": ("c32",)}


class Group:
    def __init__(self, env, key):
        ka, oracle = env.ka, env.oracle
        rng = np.random.default_rng(7 + 131 * sum(map(ord, str(key))))
        W, nh, L = ss.group_shape(key)
        self.key, self.W, self.nh, self.L = key, W, nh, L
        nrows, nb = 1 << L, (W + 7) // 8
        dense = key[0] == "count_dense"
        common = 8 if dense else 32                          # base bytes used all over the row
        p = ss.group_fill(key)
        # planted columns: (kind, rows), one base column each -- the unique base bytes follow the common ones
        planted = []
        t0s = (0.8, 0.9)
        for bk in GROUP_BATCHES[key[0]]:
            for s in env.batch(bk).plant:
                if dense:
                    planted.append(("ones", None))
                    continue
                r = env.rows(s, L)[:, :nh]
                n = r.shape[0]
                if n == 0:
                    continue
                if key[0].startswith("and"):
                    miss = r.reshape(-1)[:-1] if n == 1 else np.concatenate([r[:-1].reshape(-1), r[-1, 1:]])
                    if np.isin(r[-1, 0], miss):
                        miss = None
                    planted += [("rows", r.reshape(-1)), ("rows", miss) if miss is not None else ("none", None)]
                else:
                    counts = {n, 0} | {c for t in t0s for f in (oracle.query_threshold(t, n),) for c in (f, f - 1) if 0 < c < n}
                    planted += [("rows", r[:c].reshape(-1)) for c in sorted(counts)]
        nu = (len(planted) + 7) // 8 + 1
        assert nu < nb - common, key
        base = rand_bits(rng, (nrows, 8 * (common + nu)), p)
        base[:, 8 * common:] = False                          # unique columns: the planted rows only
        for i, (kind, r) in enumerate(planted[:2]):            # the first two planted columns also in common ones: repeated all over the row
            if kind == "rows":
                base[r, 8 * i + 3] = True
        for i, (kind, r) in enumerate(planted):
            c = 8 * common + i
            if kind == "rows":
                base[r, c] = True
            elif kind == "ones":
                base[:, c] = True
        if dense:
            base[:, :8 * common:5] = True                     # common columns of all ones too: counts of n all over the row
        # the byte map: common bytes at random, the unique ones at the row's edges
        bmap = rng.integers(0, common, size=nb)
        edges = [0, 15, 16, 127, 128, nb // 2, nb - 1] + [j for s in range(1024, nb, 1024) for j in (s - 1, s)]
        edges = list(dict.fromkeys(e for e in edges if 0 <= e < nb))
        extra = [e for e in rng.permutation(nb).tolist() if e not in edges]
        spots = (edges + extra)[:nu]
        bmap[spots] = common + np.arange(nu)
        self.cmap = (8 * np.repeat(bmap, 8) + np.tile(np.arange(8), nb))[:W]
        self.base = pack_columns(base, rng)
        self.nbase = base.shape[1]
        img = np.empty((nrows, nb + 3), dtype=np.uint8)
        img[:, :nb] = self.base[:, bmap]
        img[:, nb:] = rng.integers(0, 256, size=(nrows, 3), dtype=np.uint8)
        if W % 8:                                             # garbage in the last byte's pad bits
            keep = np.uint8((1 << (W % 8)) - 1)
            img[:, nb - 1] = (img[:, nb - 1] & keep) | (rng.integers(0, 256, size=nrows, dtype=np.uint8) & ~keep)
        self.g = ka.Group(env.ctx, K, nh, L, W)
        self.g.add_columns(img, W)
        self.g.finalize()

    def expected(self, env, batch, t):
        key = (self.key, batch.key, t)
        if key in env.expected:
            return env.expected[key]
        t32 = float(np.float32(t))
        per = {}
        for s in batch.distinct:
            km = env.oracle.unique_kmers(s, K)
            hits, _ = env.oracle.search_image(self.base, self.base.shape[1], K, self.nh, self.L, self.nbase, km, t32)
            m = np.full(self.nbase, -1, dtype=np.int64)
            if hits:
                c, v = zip(*hits)
                m[np.asarray(c)] = v
            wm = m[self.cmap]
            cols = np.flatnonzero(wm >= 0)
            per[s] = (cols, wm[cols])
        parts = []
        for q, s in enumerate(batch.seqs):
            cols, v = per[s]
            rec = np.empty(cols.size, dtype=HIT_DTYPE)
            rec["query"], rec["column"], rec["num_match"] = q, cols, v
            parts.append(rec)
        exp = np.concatenate(parts)
        env.expected[key] = exp
        return exp


def run_case(env, c, t=None, flags=None, knobs=None, exact_name=True):
    g, b = env.group(c.group), env.batch(c.batch)
    t = c.t if t is None else t
    out = []
    for fl in (c.flags if flags is None else flags):
        with env.ctx.tuning(**dict(c.knobs, **(knobs or {}))):
            r = g.g.search(b.b, t, fl)
        what = "%s t=%g flags=%d knobs=%s got %s" % (c.name, t, fl, knobs, r.search_kernel)
        if exact_name:
            assert r.search_kernel == c.name, what
        else:
            ss.launched(r.search_kernel)
        assert np.array_equal(r.num_query_kmer, b.nkmer), what
        assert_hits_equal(r.hits, g.expected(env, b, t), what)
        if any(w in r.search_kernel for w in PERSISTENT):
            left = env.ctx.scratch_nonzero()
            assert not any(left.values()), (what, left)
        out.append(r.search_kernel)
    return out


def run_family(env, test, variants=()):
    cases = [c for c in ss.CASES if c.test == test]
    reached = set()
    for c in cases:
        run_case(env, c)
        reached |= ss.launched(c.name)
        if FULL_GRID:
            for t in SWEEP:
                if t != c.t:
                    run_case(env, c, t=t, exact_name=False)
            for kn in variants:
                run_case(env, c, knobs=kn)
    want = set().union(*(ss.launched(c.name) for c in cases))
    assert reached == want and reached
    return cases


REFINE_VARIANTS = (dict(refine_list_cap=5), dict(refine_seg_rows=8), dict(refine_seg_rows=120), dict(refine_static=0))


def test_and_narrow(env):
    run_family(env, "and_narrow")


def test_and_screen_then_refine(env):
    run_family(env, "and_screen", REFINE_VARIANTS)


def test_and_walk(env):
    run_family(env, "and_walk", (dict(walk_waves=5), dict(walk_waves=3001)))


def test_and_band_walk(env):
    run_family(env, "and_band_walk", (dict(walk_waves=5), dict(walk_bands=5)))


def test_and_kernel(env):
    run_family(env, "and_kernel")


def test_count_screen_then_refine(env):
    run_family(env, "count_screen", REFINE_VARIANTS)


def test_count_walk_truncated_then_refine(env):
    run_family(env, "count_walk_trunc", (dict(refine_list_cap=5), dict(count_walk_waves=7), dict(count_walk_waves=3001)))


def test_count_walk(env):
    run_family(env, "count_walk_pf", (dict(count_walk_waves=7), dict(count_walk_waves=3001)))


def test_count_kernel(env):
    run_family(env, "count_kernel")


def test_count_segments_and_combine(env):
    run_family(env, "count_segments")


def test_count_narrow(env):
    run_family(env, "count_narrow")
