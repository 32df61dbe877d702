"""kwage_search_scores / kwage_search_scores_device (the dense score search) through the C ABI and the Python mirror.

Expected matrix: the CPU oracle's count of every column (a threshold whose floor is 0; columns it does not list count
0), 0 on pad columns and for queries without k-mers.  Every comparison is exact integer equality.  The device's own
threshold search (kwage_search at t = 0.5 and 1) is a second oracle.

(The contract's last argument error -- a query of 2^32 rows and more -- needs a query of 859 M bases at five hash
functions: like the same check of the top-k search it is not exercised here.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7


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


def make_group(ka, ctx, rng, k, num_hash, L, files_nf, density, dup_pairs, full_cols=()):
    """A group of several 'files' (add_columns), garbage in the pad bits of every image, planted duplicate columns
    (tests/test_gpu_topk.py builds its groups the same way) and, in every file, the columns `full_cols` with every bit
    set: each query scores its whole k-mer count there.  Returns (group, [(first_column, image, nf)])."""
    g = ka.Group(ctx, k, num_hash, L, sum(nf + 128 for nf in files_nf))
    files = []
    for nf in files_nf:
        bits = rng.random((1 << L, nf)) < density
        for a, b in dup_pairs:
            if a < nf and b < nf:
                bits[:, b] = bits[:, a]
        for c in full_cols:
            if c < nf:
                bits[:, c] = True
        width = (nf + 7) // 8 + 3
        img = np.zeros((1 << L, width * 8), dtype=bool)
        img[:, :nf] = bits
        img[:, nf:] = rng.random((1 << L, width * 8 - nf)) < 0.5      # pad bits: garbage
        packed = np.packbits(img, axis=1, bitorder="little")
        first = g.add_columns(packed, nf)
        files.append((first, np.ascontiguousarray(packed), nf))
    g.finalize()
    return g, files


def oracle_matrix(oracle, files, span, k, num_hash, L, queries):
    """(uint32 [n, span] expected matrix, n per query, bool [span] real columns)."""
    exp = np.zeros((len(queries), span), dtype=np.uint32)
    nk = []
    real = np.zeros(span, dtype=bool)
    for first, _, nf in files:
        real[first:first + nf] = True
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, k)
        nk.append(len(kmers))
        if not len(kmers):
            continue
        for first, img, nf in files:
            hits, _ = oracle.search_image(img, img.shape[1], k, num_hash, L, nf, kmers, 1e-12)
            for c, m in hits:
                exp[q, first + c] = m
    return exp, np.asarray(nk, dtype=np.uint32), real


def the_queries(rng, long_len=100000):
    genome = "".join(rng.choice(list("ACGT"), size=long_len + 20000))
    queries = [genome[i * 700:i * 700 + ln] for i, ln in enumerate((100, 150, 333, 1000, 640))]
    queries += ["ACGTACGTAC",                                    # shorter than k: no k-mers
                "",                                              # empty
                genome[:long_len]]                               # long: the segmented path
    return genome, queries


@pytest.mark.parametrize("num_hash", [1, 3, 5])
def test_scores_match_oracle(ka, ctx, oracle, num_hash):
    rng = np.random.default_rng(70 + num_hash)
    kmer, L = 21, 11
    density = {1: 0.35, 3: 0.7, 5: 0.82}[num_hash]
    dup_pairs = [(3, 4), (3, 900), (17, 2000), (100, 101), (5000, 5001)]
    g, files = make_group(ka, ctx, rng, kmer, num_hash, L, [3001, 9000 - 333], density, dup_pairs, full_cols=(11, 8600))
    _, queries = the_queries(rng)
    span = g.column_span
    assert span > 8192 and span % 8 == 0 and span < g.row_stride * 8          # two tiles, the last one cut by the span
    exp, nk, real = oracle_matrix(oracle, files, span, kmer, num_hash, L, queries)
    assert nk[5] == 0 and nk[6] == 0 and nk[7] > 90000 and all(exp[q].max() == nk[q] for q in range(len(queries)))
    b = ka.Batch(ctx, queries)
    try:
        # default: this small batch (fewer than 2048 tiles) takes the segmented form; force_segs=1: one wave per
        # (query, 8192-column tile); both store epilogues of each
        for segs, kernel in ((0, "count_kernel<"), (1, "score_tile_kernel<20,%d>" % num_hash), (3, "+score_combine_kernel<20>")):
            for form in (0, 1):
                with ctx.tuning(force_segs=segs, scores_form=form):
                    res = ka.search_scores(g, b, ka.SEARCH_TIMING)
                assert kernel in res.kernel, (segs, res.kernel)
                assert res.scores.dtype == np.uint32 and res.scores.shape == (len(queries), span)
                assert np.array_equal(res.num_query_kmer, nk), (segs, form)
                bad = np.argwhere(res.scores != exp)
                assert bad.size == 0, (num_hash, segs, form, res.kernel, bad[:5].tolist(),
                                       [(int(res.scores[q, c]), int(exp[q, c])) for q, c in bad[:5]])
                assert not res.scores[:, ~real].any() and not res.scores[nk == 0].any()
                assert res.kernel_ms > 0
    finally:
        b.close()
        g.close()


@pytest.fixture(scope="module")
def small(ka, ctx, oracle):
    """One group (two files, 12 k columns, 2^12 rows, three hash functions), its queries and the oracle's matrix."""
    rng = np.random.default_rng(5)
    kmer, nh, L = 21, 3, 12
    g, files = make_group(ka, ctx, rng, kmer, nh, L, [2999, 9001], 0.7, [(3, 4), (17, 2000), (2998, 8000)], full_cols=(7, 2500))
    genome, queries = the_queries(rng, 3000)
    b = ka.Batch(ctx, queries)
    exp, nk, real = oracle_matrix(oracle, files, g.column_span, kmer, nh, L, queries)
    yield dict(g=g, files=files, b=b, queries=queries, exp=exp, nk=nk, real=real, kmer=kmer, nh=nh, L=L, rng=rng, genome=genome)
    b.close()
    g.close()


def test_cells_beyond_the_span_are_untouched(ka, ctx, small):
    import torch
    from kwage_amd.native import lib, check
    g, b, exp = small["g"], small["b"], small["exp"]
    n, span = exp.shape
    for form in (0, 1):
        for segs in (1, 3):
            with ctx.tuning(scores_form=form, force_segs=segs):
                # device form: a matrix 12 cells wider than the span
                out = torch.full((n, span + 12), SENTINEL, dtype=torch.int32, device="cuda:0")
                nkd = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
                res = ka.search_scores_device(g, b, out, nkd)
                got = out.cpu().numpy()
                assert (got[:, span:] == SENTINEL).all(), (form, segs)
                assert np.array_equal(got[:, :span].view(np.uint32), exp), (form, segs, res.kernel)
                assert not got[:, :span][:, ~small["real"]].any()              # pad columns: 0, not the sentinel
                assert np.array_equal(nkd.cpu().numpy().view(np.uint32), small["nk"])
                # host form: the same through kwage_search_scores
                host = np.full((n, span + 4), SENTINEL, dtype=np.int32)
                check(lib().kwage_search_scores(g._h, b._h, host.ctypes.data, span + 4, None, 0, None))
                assert (host[:, span:] == SENTINEL).all() and np.array_equal(host[:, :span].view(np.uint32), exp), (form, segs)


def test_scores_agree_with_the_threshold_search(ka, ctx, small):
    g, b, nk, real = small["g"], small["b"], small["nk"], small["real"]
    scores = ka.search_scores(g, b).scores
    for t in (0.5, 1.0):
        thr = g.search(b, t)
        assert np.array_equal(thr.num_query_kmer, nk)
        h = thr.hits
        assert h.size and np.array_equal(scores[h["query"], h["column"]], h["num_match"]), t
        if t == 0.5:
            # (kwage_search lists nothing for a query without k-mers; its row here is all zeros)
            mine = {(q, c) for q in np.flatnonzero(nk) for c in np.flatnonzero(real & (scores[q] >= thr.query_threshold[q]))}
            assert mine == set(zip(h["query"].tolist(), h["column"].tolist()))


def test_host_and_device_forms_agree(ka, ctx, oracle, small):
    import torch
    g, b, exp, queries = small["g"], small["b"], small["exp"], small["queries"]
    kmer, nh, L = small["kmer"], small["nh"], small["L"]
    n, span = exp.shape
    host = ka.search_scores(g, b)
    out = torch.full((n, span), SENTINEL, dtype=torch.int32, device="cuda:0")
    dev = ka.search_scores_device(g, b, out)
    assert dev.kernel == host.kernel and dev.num_query_kmer is None
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host.scores) and np.array_equal(host.scores, exp)

    # two groups side by side in one matrix (the second with other parameters)
    rng = np.random.default_rng(6)
    g2, files2 = make_group(ka, ctx, rng, kmer, 1, 11, [777, 1500], 0.4, [(1, 2)])
    try:
        exp2, _, _ = oracle_matrix(oracle, files2, g2.column_span, kmer, 1, 11, queries)
        both = ka.Database([g, g2]).search_scores(b)
        assert tuple(both.shape) == (n, span + g2.column_span) and both.dtype == torch.int32
        got = both.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:, :span], exp) and np.array_equal(got[:, span:], exp2)
        assert np.array_equal(got[:, span:], ka.search_scores(g2, b).scores)
    finally:
        g2.close()


def test_sparse_group_gives_the_full_groups_matrix(ka, ctx, small):
    g, b, files, exp = small["g"], small["b"], small["files"], small["exp"]
    kmer, nh, L = small["kmer"], small["nh"], small["L"]
    _, rows = ka.hash_batch(ctx, kmer, nh, L, b)
    need = np.unique(np.concatenate([r.reshape(-1) for r in rows]))
    sp = ka.Group.sparse(ctx, kmer, nh, L, sum(nf + 128 for _, _, nf in files), need)
    other = ka.Batch(ctx, ["".join(small["rng"].choice(list("ACGT"), size=400))])
    try:
        for first, img, nf in files:
            assert sp.add_columns(np.ascontiguousarray(img[need]), nf) == first
        sp.finalize()
        assert sp.column_span == g.column_span
        for segs in (1, 3):
            with ctx.tuning(force_segs=segs):
                full, part = ka.search_scores(g, b), ka.search_scores(sp, b)
            assert part.kernel == full.kernel and np.array_equal(part.scores, full.scores) and np.array_equal(full.scores, exp)
            assert np.array_equal(part.num_query_kmer, full.num_query_kmer)
        # a sparse group made for other queries: refused, nothing written
        import torch
        out = torch.full((1, sp.column_span), SENTINEL, dtype=torch.int32, device="cuda:0")
        with pytest.raises(ka.KwageError) as ei:
            ka.search_scores_device(sp, other, out)
        assert ei.value.code == -6 and "not among the rows" in str(ei.value), ei.value
        assert (out.cpu().numpy() == SENTINEL).all()
        assert np.array_equal(ka.search_scores(sp, b).scores, exp)              # still gives the right matrix
    finally:
        other.close()
        sp.close()


def test_argument_errors_leave_the_buffer_untouched(ka, small):
    import torch
    from kwage_amd.native import lib
    g, b, exp = small["g"], small["b"], small["exp"]
    n, span = exp.shape
    out = torch.full((n * (span + 8) + 8,), SENTINEL, dtype=torch.int32, device="cuda:0")
    host = np.full(n * (span + 8), SENTINEL, dtype=np.int32)
    other_ctx = ka.Context(0)
    foreign = ka.Batch(other_ctx, small["queries"])
    unfinished = ka.Group(small["b"].ctx, small["kmer"], small["nh"], small["L"], 1000)
    unfinished.add_random_columns(1000, 3, 64)

    def call(group, batch, ptr, row_elems, host_form=False):
        fn = lib().kwage_search_scores if host_form else lib().kwage_search_scores_device
        return fn(group._h, batch._h, ptr, row_elems, None, 0, None)
    try:
        p = out.data_ptr()
        assert p % 16 == 0
        cases = [("row_elems below the span", g, b, p, span - 4, -1),
                 ("row_elems not a multiple of 4", g, b, p, span + 2, -1),
                 ("misaligned pointer", g, b, p + 4, span, -1),
                 ("misaligned pointer", g, b, p + 8, span + 8, -1),
                 ("no matrix", g, b, None, span, -1),
                 ("mixed contexts", g, foreign, p, span, -1),
                 ("before finalize", unfinished, b, p, unfinished.column_span, -6)]
        for what, group, batch, ptr, row_elems, code in cases:
            assert call(group, batch, ptr, row_elems) == code, what
            assert lib().kwage_last_error(), what
            assert (out.cpu().numpy() == SENTINEL).all(), what
        for what, group, batch, row_elems, code in (("row_elems below the span", g, b, span - 4, -1), ("row_elems not a multiple of 4", g, b, span + 2, -1),
                                                     ("mixed contexts", g, foreign, span, -1), ("before finalize", unfinished, b, unfinished.column_span, -6)):
            assert call(group, batch, host.ctypes.data, row_elems, host_form=True) == code, what
            assert (host == SENTINEL).all(), what
        with pytest.raises(ValueError):
            ka.search_scores_device(g, b, out[:n * span].view(n, span).to(torch.int64))
        with pytest.raises(ValueError):
            ka.search_scores_device(g, b, out[:n * (span - 8)].view(n, span - 8))
        # and a valid call on the same buffer afterwards: rows span + 8 apart
        view = out[:n * (span + 8)].view(n, span + 8)[:, :span]
        ka.search_scores_device(g, b, view)
        assert np.array_equal(view.cpu().numpy().view(np.uint32), exp)
    finally:
        unfinished.close()
        foreign.close()
        other_ctx.close()
