"""kwage_topk_merge_device (the device merge of top-k lists) and kwage_search_topk_device_append, through the C ABI and
the Python mirror.

The merge is checked against a numpy statement of its contract: per query the first k records under (num_match
descending, order[column] ascending), listed by (query, column).  The append form and Database.search_topk are checked
against kwage_search_topk itself: one group's columns split into three groups inside 8192-column tiles, with equal
columns planted across the splits, must give back the whole group's selection."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def ctx(ka):
    c = ka.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _expected(q, c, m, k, order=None):
    """The contract: rows (query, column, num_match) ordered by (query, column)."""
    tie = c if order is None else order[c]
    idx = np.lexsort((tie, -m.astype(np.int64), q))
    qs = q[idx]
    starts = np.searchsorted(qs, qs, side="left")
    keep = idx[(np.arange(len(idx)) - starts) < k]
    out = np.stack([q[keep], c[keep], m[keep]], axis=1).astype(np.uint32)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def _records(rng, n_queries, n_cols, per_query, max_score):
    """Distinct (query, column) pairs, per_query[q] of them for query q, scores in [0, max_score] (many ties)."""
    q = np.repeat(np.arange(n_queries, dtype=np.uint32), per_query)
    c = np.empty(len(q), dtype=np.uint32)
    at = 0
    for i, n in enumerate(per_query):
        if n:
            c[at:at + n] = rng.choice(n_cols, size=n, replace=False) if n * 4 > n_cols else \
                np.unique(rng.integers(0, n_cols, size=2 * n + 16))[:n]
            at += n
    m = rng.integers(0, max_score + 1, size=len(q)).astype(np.uint32)
    assert len(np.unique(q.astype(np.uint64) << 32 | c)) == len(q)
    return q, c, m


def _merge(ka, ctx, torch, q, c, m, n_queries, k, order=None):
    rows = torch.from_numpy(np.stack([q, c, m], axis=1).astype(np.uint32).view(np.int32)).cuda()
    ordt = None if order is None else torch.from_numpy(order.astype(np.uint32).view(np.int32)).cuda()
    out = ka.merge_topk_device(ctx, rows, n_queries, k, ordt)
    return out.cpu().numpy().view(np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("k", [1, 7, 64, 1024])
def test_merge_matches_contract_with_order_table_ties_and_shuffles(ka, ctx, torch, k):
    rng = np.random.default_rng(100 + k)
    n_queries, n_cols = 240, 60000
    per_query = rng.integers(0, 2500, size=n_queries)
    per_query[::7] = 0                                     # queries with no records
    per_query[3] = 1
    q, c, m = _records(rng, n_queries, n_cols, per_query, 12)
    order = rng.permutation(n_cols).astype(np.uint32)      # order != column
    for tie in (None, order):
        exp = _expected(q, c, m, k, tie)
        # several sources: four lists, each in its own order, concatenated
        srcs = np.array_split(rng.permutation(len(q)), 4)
        idx = np.concatenate([np.sort(s) for s in srcs])
        got = _merge(ka, ctx, torch, q[idx], c[idx], m[idx], n_queries, k, tie)
        assert np.array_equal(got, exp), (k, tie is None)
        perm = rng.permutation(len(q))                     # shuffled input: the same output
        got2 = _merge(ka, ctx, torch, q[perm], c[perm], m[perm], n_queries, k, tie)
        assert np.array_equal(got2, exp)
    counts = np.bincount(exp[:, 0], minlength=n_queries)
    assert np.array_equal(counts, np.minimum(per_query, k))


def test_merge_large_bucket_and_many_queries(ka, ctx, torch):
    rng = np.random.default_rng(5)
    # one query's bucket holds 150 000 records among a few small ones
    per_query = np.array([40, 150000, 0, 3000, 9])
    q, c, m = _records(rng, len(per_query), 1 << 20, per_query, 30)
    order = rng.permutation(1 << 20).astype(np.uint32)
    for k in (10, 1024):
        got = _merge(ka, ctx, torch, q, c, m, len(per_query), k, order)
        assert np.array_equal(got, _expected(q, c, m, k, order)), k
    # 100 000 queries at k = 10, about 25 records each (two lists of ~12 per query)
    n_queries = 100000
    per_query = rng.integers(0, 50, size=n_queries)
    q = np.repeat(np.arange(n_queries, dtype=np.uint32), per_query)
    c = (rng.integers(0, 1 << 12, size=len(q)).astype(np.uint32) << 8) | (np.arange(len(q)) % 256).astype(np.uint32)
    pair = q.astype(np.uint64) << 32 | c
    _, first = np.unique(pair, return_index=True)
    q, c = q[first], c[first]
    m = rng.integers(0, 8, size=len(q)).astype(np.uint32)
    perm = rng.permutation(len(q))
    got = _merge(ka, ctx, torch, q[perm], c[perm], m[perm], n_queries, 10)
    assert np.array_equal(got, _expected(q, c, m, 10))


def test_merge_argument_errors_are_reported_not_faulted(ka, ctx, torch):
    from kwage_amd import native
    from kwage_amd.native import lib
    rng = np.random.default_rng(9)
    q, c, m = _records(rng, 20, 1000, rng.integers(1, 50, size=20), 5)
    for k in (0, ka.TOPK_MAX + 1):
        with pytest.raises(ka.KwageError) as e:
            _merge(ka, ctx, torch, q, c, m, 20, k)
        assert e.value.code == -1
    with pytest.raises(ka.KwageError) as e:                # a query index >= n_queries, found on the device
        _merge(ka, ctx, torch, q, c, m, 19, 5)
    assert e.value.code == -1 and "n_queries" in e.value.message
    with pytest.raises(ka.KwageError) as e:                # a column beyond the order table
        _merge(ka, ctx, torch, q, c, m, 20, 5, np.arange(int(c.max()), dtype=np.uint32))
    assert e.value.code == -1 and "order table" in e.value.message
    # the context still works after the reported errors
    assert np.array_equal(_merge(ka, ctx, torch, q, c, m, 20, 5), _expected(q, c, m, 5))
    # NULL pointers and a too small output, through the C ABI
    rows = torch.from_numpy(np.stack([q, c, m], axis=1).astype(np.uint32).view(np.int32)).cuda()
    out = torch.empty((100, 3), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L = lib()
    assert L.kwage_topk_merge_device(None, rows.data_ptr(), len(q), 20, 5, None, 0, out.data_ptr(), 100, cnt.data_ptr()) == -1
    assert L.kwage_topk_merge_device(ctx._h, None, len(q), 20, 5, None, 0, out.data_ptr(), 100, cnt.data_ptr()) == -1
    assert L.kwage_topk_merge_device(ctx._h, rows.data_ptr(), len(q), 20, 5, None, 0, None, 100, cnt.data_ptr()) == -1
    assert L.kwage_topk_merge_device(ctx._h, rows.data_ptr(), len(q), 20, 5, None, 0, out.data_ptr(), 100, None) == -1
    exp = _expected(q, c, m, 5)
    assert len(exp) > 60
    assert L.kwage_topk_merge_device(ctx._h, rows.data_ptr(), len(q), 20, 5, None, 0, out.data_ptr(), 60, cnt.data_ptr()) == -1
    assert int(cnt.item()) == len(exp)
    assert np.array_equal(out[:60].cpu().numpy().view(np.uint32), exp[:60])
    # nothing in, nothing out
    assert L.kwage_topk_merge_device(ctx._h, None, 0, 20, 5, None, 0, None, 0, cnt.data_ptr()) == 0
    assert int(cnt.item()) == 0
    assert native.TOPK_MAX == 1024


# ---- one group split into three: the append form, the merge, Database.search_topk ------------------------------------

SPLITS = (0, 5000, 13000, 20000)          # 5000 and 13000 lie inside the first two 8192-column tiles


def _image(rng, n_rows, n_cols, density):
    bits = rng.random((n_rows, n_cols)) < density
    for a, b in ((17, 6001), (17, 15000), (4999, 5000), (12999, 13000), (300, 19000), (8191, 8192)):
        bits[:, b] = bits[:, a]                            # equal columns on both sides of the splits and tile edges
    return bits


def _group(ka, ctx, kmer, nh, L, bits):
    n = bits.shape[1]
    width = (n + 7) // 8
    img = np.zeros((bits.shape[0], width * 8), dtype=bool)
    img[:, :n] = bits
    g = ka.Group(ctx, kmer, nh, L, n + 128)
    assert g.add_columns(np.ascontiguousarray(np.packbits(img, axis=1, bitorder="little")), n) == 0
    g.finalize()
    return g


@pytest.fixture(scope="module")
def split_case(ka, ctx):
    rng = np.random.default_rng(21)
    kmer, nh, L = 15, 2, 10
    bits = _image(rng, 1 << L, SPLITS[-1], 0.35)
    whole = _group(ka, ctx, kmer, nh, L, bits)
    parts = [_group(ka, ctx, kmer, nh, L, bits[:, a:b]) for a, b in zip(SPLITS, SPLITS[1:])]
    seqs = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(20, 160, size=37)] + ["ACG", "ACGTA"]
    b = ka.Batch(ctx, seqs)
    yield whole, parts, b
    b.close()
    for g in [whole] + parts:
        g.close()


def _rows(res):
    return np.stack([res.hits["query"], res.hits["column"], res.hits["num_match"]], axis=1).astype(np.uint32)


@pytest.mark.parametrize("t", [0.0, 0.8, 1.0])
def test_split_groups_merge_to_the_whole_groups_topk(ka, ctx, torch, split_case, t):
    whole, parts, b = split_case
    for k in (3, 64):
        exp = _rows(ka.search_topk(whole, b, k, t))
        hits = torch.empty((3 * b.n * k, 3), dtype=torch.int32, device="cuda")
        cnt = torch.empty(1, dtype=torch.int64, device="cuda")
        n = 0
        for i, (g, base) in enumerate(zip(parts, SPLITS)):
            n = ka.search_topk_device_append(g, b, k, hits, cnt, base, t, reset=(i == 0))
        assert n == int(cnt.item())
        got = ka.merge_topk_device(ctx, hits[:n], b.n, k).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), (t, k)
        if t == 0.0:
            assert len(exp) == (b.n - 2) * k               # the last two queries have no 15-mers


def test_append_is_search_topk_plus_base_behind_existing_records(ka, ctx, torch, split_case):
    whole, parts, b = split_case
    g, k, t = parts[1], 20, 0.0
    exp = _rows(ka.search_topk(g, b, k, t))
    hits = torch.full((3 * len(exp) + 10, 3), -1, dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    nk = torch.zeros(b.n, dtype=torch.int32, device="cuda")
    n1 = ka.search_topk_device_append(g, b, k, hits, cnt, 0, t, reset=True, num_query_kmer=nk)
    assert n1 == len(exp)
    assert np.array_equal(nk.cpu().numpy().view(np.uint32), ka.search_topk(g, b, k, t).num_query_kmer)
    n2 = ka.search_topk_device_append(g, b, k, hits, cnt, 70000, t, reset=False)
    assert n2 == 2 * len(exp) and int(cnt.item()) == n2
    got = hits[:n2].cpu().numpy().view(np.uint32)
    shifted = exp.copy()
    shifted[:, 1] += 70000
    assert np.array_equal(got[:n1], exp) and np.array_equal(got[n1:], shifted)
    assert (hits[n2:].cpu().numpy() == -1).all()           # nothing written behind the list
    # reset starts over
    assert ka.search_topk_device_append(g, b, k, hits, cnt, 5, t, reset=True) == len(exp)
    # past the capacity: counted, not stored
    small = torch.full((len(exp) // 2 + 1, 3), -1, dtype=torch.int32, device="cuda")
    assert ka.search_topk_device_append(g, b, k, small, cnt, 0, t, reset=True) == len(exp)
    assert np.array_equal(small.cpu().numpy().view(np.uint32), exp[:small.shape[0]])
    with pytest.raises(ka.KwageError):
        ka.search_topk_device_append(g, b, 0, hits, cnt, 0, t)
    with pytest.raises(ka.KwageError):
        ka.search_topk_device_append(g, b, k, hits, cnt, 0xFFFFFF00, t)     # base + span beyond 32 bits


def test_database_search_topk_is_the_host_merge_over_groups_of_two_parameter_sets(ka, ctx, split_case):
    whole, parts, b = split_case
    rng = np.random.default_rng(33)
    other = [_group(ka, ctx, 11, 1, 9, rng.random((1 << 9, n)) < 0.3) for n in (700, 9000)]
    groups = [parts[0], other[0], parts[2], other[1]]
    db = ka.Database(groups)
    for k, t in ((1, 0.0), (16, 0.0), (16, 0.5)):
        got = db.search_topk(b, k, t)
        per_q = [[] for _ in range(b.n)]
        for gi, g in enumerate(groups):
            for q, c, m in ka.search_topk(g, b, k, t).hits.tolist():
                per_q[q].append((gi, c, m))
        exp = [sorted(lst, key=lambda h: (-h[2], h[0], h[1]))[:k] for lst in per_q]
        assert got == exp, (k, t)
    for g in other:
        g.close()


def test_merge_more_queries_than_one_grid_and_long_runs(ka, ctx, torch):
    """More queries than the select kernel's grid (2^20 workgroups: the grid loops over the rest), and records in long runs
    of one query -- the order an exchange delivers them in, where the count and scatter passes take one atomic per run --
    interleaved with runs cut short by a record of another query."""
    rng = np.random.default_rng(77)
    n_queries = (1 << 20) + 5000
    qs = np.sort(rng.choice(n_queries, size=30000, replace=False)).astype(np.uint32)
    qs[-1] = n_queries - 1                                 # the last query: reached only by the grid's loop
    per = rng.integers(1, 200, size=len(qs))
    q = np.repeat(qs, per)
    c = np.concatenate([rng.choice(1 << 16, size=n, replace=False) for n in per]).astype(np.uint32)
    m = rng.integers(0, 20, size=len(q)).astype(np.uint32)
    # two sources, each ordered by query: a record of the other source every few records breaks the runs
    src = rng.random(len(q)) < 0.1
    idx = np.concatenate([np.nonzero(~src)[0], np.nonzero(src)[0]])
    for k in (3, 100):
        got = _merge(ka, ctx, torch, q[idx], c[idx], m[idx], n_queries, k)
        assert np.array_equal(got, _expected(q, c, m, k)), k
