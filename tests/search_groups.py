"""What test_gpu_search_shapes.py and test_gpu_search_holes.py share: the context, batches and groups of the case tables
(search_shapes.py, search_holes.py), the oracle's expectation and the run of one case.

Wide groups stay cheap for the oracle: a group is made of copies of a narrow base block.  Byte j of every row is base byte
map[j], drawn at random (not periodic in 128 or 1024 columns), so column j is base column 8 map[j] + j % 8; a few base
bytes are used once only, at the first, middle and last 128-byte group and at KiB-step boundaries
(search_shapes.planted_edges), and hold the planted columns: every row of a query (count n), the rows of its first thr and
thr - 1 distinct k-mers, none (count 0), and at t = 1 all but one row of one k-mer.  The oracle counts the base; the map
spreads its lists over the group.  Pad bits hold garbage.

What depends on the sequences and the group key alone -- a query's rows, the oracle's list of a (group, batch, threshold)
-- is computed once per process, whichever file asks first."""
import os

import numpy as np

import search_shapes as ss
from topk_reference import HIT_DTYPE, assert_hits_equal, pack_columns, rand_bits

FULL_GRID = os.environ.get("KWAGE_SEARCH_FULL_GRID", "0") == "1"
SWEEP = (1.0, 0.9, 0.8, 0.5, 0.05)
K = ss.K
PERSISTENT = ("walk", "screen", "trunc", "refine")

_ROWS, _NKMER, _EXPECTED = {}, {}, {}          # per process: (seq, L) -> rows, seq -> distinct k-mers, (ncu, group, batch, t) -> list


class Env:
    """A module's context, groups and batches, built on first use and shared by its tests.  `group`: the class its groups
    are made with."""

    def __init__(self, ka, oracle, group=None):
        self.ka, self.oracle = ka, oracle
        self.ctx = ka.Context(0)
        self.ncu = int(self.ctx.fingerprint()["cus"])
        self.group_class = group or Group
        self.groups, self.batches = {}, {}
        self.expected = _EXPECTED.setdefault(self.ncu, {})
        self.rows_cache = _ROWS

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
            self.groups[key] = self.group_class(self, key)
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
        for s in self.distinct:
            if s not in _NKMER:
                _NKMER[s] = len(env.oracle.unique_kmers(s, K))
        self.nkmer = np.array([_NKMER[s] for s in seqs], dtype=np.uint32)


GROUP_BATCHES = {"and": ("and",), "and_wide": ("and_wide",), "and_narrow": ("and_short",), "count": ("c7", "c10", "c14a", "c14b", "c20a", "c20b", "c32r"),
                 "count_narrow": ("n7", "n10", "n14"), "count_dense": ("c32",), "count_wide": ("c10", "c14a")}


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
        edges = ss.planted_edges(nb)
        extra = [e for e in rng.permutation(nb).tolist() if e not in edges]
        spots = (edges + extra)[:nu]
        bmap[spots] = common + np.arange(nu)
        self.spots = spots
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
        self.load(env, img)

    def load(self, env, img):
        """The image becomes the resident group."""
        self.g.add_columns(img, self.W)
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

    def check_hits(self, hits, what):
        """What a group asserts of a hit list beyond its equality with expected()."""


def run_case(env, c, t=None, flags=None, knobs=None, exact_name=True):
    g, b = env.group(c.group), env.batch(c.batch)
    t = c.t if t is None else t
    exp = g.expected(env, b, t)                  # (the reference first: what it asserts of itself does not wait for the device)
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
        g.check_hits(r.hits, what)
        assert_hits_equal(r.hits, exp, what)
        if any(w in r.search_kernel for w in PERSISTENT):
            left = env.ctx.scratch_nonzero()
            assert not any(left.values()), (what, left)
        out.append(r.search_kernel)
    return out


def run_family(env, table, test):
    """Every case of `table` that belongs to `test` (KWAGE_SEARCH_FULL_GRID=1: with the threshold sweep and the knob variants
    of VARIANTS); at the end the test has reached every instantiation its cases name."""
    cases = [c for c in table if c.test == test]
    variants = VARIANTS[test]
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
# (test of the case tables -> the knob variants KWAGE_SEARCH_FULL_GRID=1 adds to each of its cases)
VARIANTS = {"and_narrow": (), "and_screen": REFINE_VARIANTS, "and_walk": (dict(walk_waves=5), dict(walk_waves=3001)),
            "and_band_walk": (dict(walk_waves=5), dict(walk_bands=5)), "and_kernel": (), "count_screen": REFINE_VARIANTS,
            "count_walk_trunc": (dict(refine_list_cap=5), dict(count_walk_waves=7), dict(count_walk_waves=3001)),
            "count_walk_pf": (dict(count_walk_waves=7), dict(count_walk_waves=3001)), "count_kernel": (), "count_segments": (), "count_narrow": ()}
