"""kwage_search_filter_scores / _device, kwage_group_column_bits and Database.similar: whole Bloom filters scored
against every column of a group.

Expected cell (i, c): the number of rows set in both filter i and column c of the host image the test itself loaded --
the popcount of filter & column (expected() below).  0 on pad columns.  Every comparison of cells is exact integer equality."""
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


def rand_bits(rng, shape, density):
    """bool array of i.i.d. bits; at density 0.5 from random bytes (an eighth of the generator's work: the 2^20-row groups)."""
    if density == 0.5:
        n = int(np.prod(shape))
        return np.unpackbits(rng.integers(0, 256, size=(n + 7) // 8, dtype=np.uint8))[:n].astype(bool).reshape(shape)
    return rng.random(shape) < density


def make_group(ka, ctx, rng, k, num_hash, L, files_nf, density, dup_pairs=(), full_cols=()):
    """A group of several 'files' (add_columns), garbage in the pad bits of every image, planted duplicate columns and
    full columns, built the way tests/test_gpu_scores.py builds its groups.  Returns (group, [(first_column, image, nf)])."""
    g = ka.Group(ctx, k, num_hash, L, sum(nf + 128 for nf in files_nf))
    files = []
    for nf in files_nf:
        bits = rand_bits(rng, (1 << L, nf), density)
        for a, b in dup_pairs:
            if a < nf and b < nf:
                bits[:, b] = bits[:, a]
        for c in full_cols:
            if c < nf:
                bits[:, c] = True
        width = (nf + 7) // 8 + 3
        img = np.zeros((1 << L, width * 8), dtype=bool)
        img[:, :nf] = bits
        img[:, nf:] = rand_bits(rng, (1 << L, width * 8 - nf), 0.5)      # pad bits: garbage
        packed = np.packbits(img, axis=1, bitorder="little")
        first = g.add_columns(packed, nf)
        files.append((first, np.ascontiguousarray(packed), nf))
    g.finalize()
    return g, files


def columns_of(files, span):
    """(bool [rows, span] matrix of the group's real columns -- pad columns all zero --, bool [span] real)."""
    nrows = files[0][1].shape[0]
    m = np.zeros((nrows, span), dtype=bool)
    real = np.zeros(span, dtype=bool)
    for first, img, nf in files:
        m[:, first:first + nf] = np.unpackbits(img[:, :(nf + 7) // 8], axis=1, bitorder="little")[:, :nf]
        real[first:first + nf] = True
    return m, real


def expected(filters01, cols01):
    """uint32 [n, span]: popcount(filter & column) for all pairs -- filter by filter, or for many filters as the product
    of the two 0/1 matrices in float64 (sums of at most 2^20 ones: exact)."""
    filters01 = np.asarray(filters01, dtype=bool)
    if filters01.shape[0] <= 16:
        return np.stack([(cols01 & f[:, None]).sum(axis=0) for f in filters01]).astype(np.uint32)
    return np.rint(filters01.astype(np.float64) @ cols01.astype(np.float64)).astype(np.uint32)


def pack_filters(f01):
    return np.packbits(np.asarray(f01, dtype=bool), axis=1, bitorder="little")


def filter_with(rng, nrows, count):
    f = np.zeros(nrows, dtype=bool)
    f[rng.choice(nrows, size=count, replace=False)] = True
    return f


# ---- the counter widths: both sides of every edge ---------------------------------------------------------------------

@pytest.mark.parametrize("L,count,planes", [(7, 127, 7), (7, 128, 10), (10, 1023, 10), (10, 1024, 14), (14, 16383, 14), (14, 16384, 20),
                                            (20, (1 << 20) - 1, 20), (20, 1 << 20, 32)])
def test_counter_width_edges(ka, ctx, L, count, planes):
    rng = np.random.default_rng(L * 100 + planes)
    nfs = [64] if L == 20 else [70, 50]          # (L = 20: 64 columns, 128 MB on the device)
    g, files = make_group(ka, ctx, rng, 21, 3, L, nfs, 0.5, full_cols=(2,))
    try:
        span = g.column_span
        cols01, real = columns_of(files, span)
        f01 = np.stack([filter_with(rng, 1 << L, count), filter_with(rng, 1 << L, max(count // 3, 1))])
        exp = expected(f01, cols01)
        assert exp[0, files[0][0] + 2] == count                   # the full column holds the whole filter
        fs = ka.FilterSet.from_bits(ctx, 21, 3, L, pack_filters(f01))
        try:
            assert fs.bit_counts().tolist() == [count, max(count // 3, 1)]
            for segs in (0, 1):
                with ctx.tuning(force_segs=segs):
                    res = ka.search_filter_scores(g, fs, ka.SEARCH_TIMING)
                # the one-hash instantiations, at the narrowest width that holds the longest filter
                if res.kernel.startswith("score_tile_kernel"):
                    assert res.kernel == "score_tile_kernel<%d,1>" % planes, res.kernel
                else:
                    assert res.kernel.startswith("count_kernel<") and ",1>+score_combine_kernel<%d>" % planes in res.kernel, res.kernel
                if segs == 1:
                    assert res.kernel.startswith("score_tile_kernel")
                bad = np.argwhere(res.scores != exp)
                assert bad.size == 0, (L, count, segs, res.kernel, bad[:5].tolist(), [(int(res.scores[q, c]), int(exp[q, c])) for q, c in bad[:5]])
                assert not res.scores[:, ~real].any() and res.kernel_ms > 0
        finally:
            fs.close()
    finally:
        g.close()


# ---- both launch forms -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many(ka, ctx):
    """2100 columns over 128 rows in two files, with duplicate and full columns; every real column as a filter."""
    rng = np.random.default_rng(21)
    g, files = make_group(ka, ctx, rng, 19, 2, 7, [1500, 600], 0.45, dup_pairs=[(3, 4), (10, 1400)], full_cols=(9,))
    span = g.column_span
    cols01, real = columns_of(files, span)
    own = np.flatnonzero(real)
    fs = ka.FilterSet.from_columns(g, own)
    exp = expected(cols01[:, own].T, cols01)
    yield dict(g=g, files=files, span=span, cols01=cols01, real=real, own=own, fs=fs, exp=exp)
    fs.close()
    g.close()


def test_many_filters_take_the_tile_form(ka, ctx, many):
    g, fs, exp, own = many["g"], many["fs"], many["exp"], many["own"]
    assert len(fs) == 2100 and len(fs) >= 2048
    for form in (0, 1):
        with ctx.tuning(scores_form=form):
            res = ka.search_filter_scores(g, fs)
        assert res.kernel == "score_tile_kernel<10,1>", res.kernel           # (a full column: 128 rows)
        assert np.array_equal(res.scores, exp), form
    # identities: own cell == the filter's bit count == the column's bit count; the matrix of own columns is symmetric
    sq = res.scores[:, own]
    assert np.array_equal(np.diagonal(sq), fs.bit_counts())
    assert np.array_equal(g.column_bits()[own], fs.bit_counts()) and not g.column_bits()[~many["real"]].any()
    assert np.array_equal(g.column_bits(), many["cols01"].sum(axis=0).astype(np.uint32))
    assert np.array_equal(sq, sq.T)


@pytest.mark.parametrize("segs", [0, 2, 3, 7])
def test_few_filters_take_segments_and_combine(ka, ctx, many, segs):
    g, files, cols01 = many["g"], many["files"], many["cols01"]
    cols = [files[0][0] + 9, files[0][0] + 3, files[1][0] + 599, files[0][0] + 4]       # the full column first: 128 rows
    fs = ka.FilterSet.from_columns(g, cols)
    try:
        exp = expected(cols01[:, cols].T, cols01)
        for form in (0, 1):
            with ctx.tuning(force_segs=segs, scores_form=form):
                res = ka.search_filter_scores(g, fs)
            assert res.kernel.startswith("count_kernel<7,1>+score_combine_kernel<10>"), (segs, res.kernel)
            assert np.array_equal(res.scores, exp), (segs, form)
        assert np.array_equal(res.scores[1], res.scores[3])                      # duplicate columns: the same row
    finally:
        fs.close()


def test_rows_wider_than_one_tile(ka, ctx):
    rng = np.random.default_rng(31)
    g, files = make_group(ka, ctx, rng, 21, 1, 8, [8192 + 200], 0.3)
    try:
        span = g.column_span
        assert span > 8192 and g.row_stride * 8 > 8192
        cols01, real = columns_of(files, span)
        cols = [0, 8191, 8192, 8192 + 199, 77]
        fs = ka.FilterSet.from_columns(g, cols)
        try:
            exp = expected(cols01[:, cols].T, cols01)
            for form in (0, 1):
                for segs in (0, 1):
                    with ctx.tuning(scores_form=form, force_segs=segs):
                        res = ka.search_filter_scores(g, fs)
                    assert np.array_equal(res.scores, exp), (form, segs, res.kernel)
            assert np.array_equal(g.column_bits(), cols01.sum(axis=0).astype(np.uint32))
        finally:
            fs.close()
    finally:
        g.close()


# ---- several groups, the contract's edges ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair(ka, ctx):
    """Group A (two files) and group B with A's parameters, group C with another hash count; filters from A's columns."""
    rng = np.random.default_rng(55)
    ga, fa = make_group(ka, ctx, rng, 21, 2, 9, [300, 41], 0.4, dup_pairs=[(1, 2), (5, 40)])
    gb, fb = make_group(ka, ctx, rng, 21, 2, 9, [150, 33], 0.6)
    gc, fc = make_group(ka, ctx, rng, 21, 3, 9, [90], 0.5)
    ca, ra = columns_of(fa, ga.column_span)
    cb, rb = columns_of(fb, gb.column_span)
    cols = [fa[0][0] + 1, fa[0][0] + 2, fa[0][0] + 299, fa[1][0] + 0, fa[1][0] + 40]
    fs = ka.FilterSet.from_columns(ga, cols)
    yield dict(ga=ga, gb=gb, gc=gc, fa=fa, fb=fb, ca=ca, cb=cb, ra=ra, rb=rb, cols=cols, fs=fs)
    fs.close()
    for g in (ga, gb, gc):
        g.close()


def test_a_set_from_one_group_searches_another(ka, ctx, pair):
    import torch
    ga, gb, gc, fs, cols = pair["ga"], pair["gb"], pair["gc"], pair["fs"], pair["cols"]
    f01 = pair["ca"][:, cols].T
    exp_a, exp_b = expected(f01, pair["ca"]), expected(f01, pair["cb"])
    assert np.array_equal(ka.search_filter_scores(ga, fs).scores, exp_a)
    assert np.array_equal(ka.search_filter_scores(gb, fs).scores, exp_b)
    # both side by side in one device matrix, pad columns 0 and not the sentinel
    sa, sb = ga.column_span, gb.column_span
    out = torch.full((len(cols), sa + sb + 12), SENTINEL, dtype=torch.int32, device="cuda:0")
    ka.search_filter_scores_device(ga, fs, out[:, :sa])
    ka.search_filter_scores_device(gb, fs, out[:, sa:sa + sb])
    got = out.cpu().numpy()
    assert (got[:, sa + sb:] == SENTINEL).all()
    assert np.array_equal(got[:, :sa].view(np.uint32), exp_a) and np.array_equal(got[:, sa:sa + sb].view(np.uint32), exp_b)
    assert not got[:, :sa][:, ~pair["ra"]].any() and not got[:, sa:sa + sb][:, ~pair["rb"]].any()
    # unequal parameters: refused, nothing written
    out.fill_(SENTINEL)
    with pytest.raises(ka.KwageError) as ei:
        ka.search_filter_scores_device(gc, fs, out[:, :gc.column_span])
    assert ei.value.code == -1 and "not comparable" in str(ei.value)
    assert (out.cpu().numpy() == SENTINEL).all()


def test_argument_errors_leave_the_buffer_untouched(ka, ctx, pair):
    import torch
    from kwage_amd.native import lib
    ga, fs, fa = pair["ga"], pair["fs"], pair["fa"]
    n, span = len(fs), ga.column_span
    out = torch.full((n * (span + 8) + 8,), SENTINEL, dtype=torch.int32, device="cuda:0")
    host = np.full(n * (span + 8), SENTINEL, dtype=np.int32)
    other_ctx = ka.Context(0)
    foreign = ka.FilterSet.from_bits(other_ctx, 21, 2, 9, np.full((1, 64), 255, dtype=np.uint8))
    unfinished = ka.Group(ctx, 21, 2, 9, 256)
    unfinished.add_columns(fa[1][1], fa[1][2])
    listed = np.arange(0, 512, 2, dtype=np.uint32)
    sparse = ka.Group.sparse(ctx, 21, 2, 9, 256, listed)
    sparse.add_columns(np.ascontiguousarray(fa[1][1][listed]), fa[1][2])
    sparse.finalize()

    def call(group, fset, ptr, row_elems, host_form=False):
        fn = lib().kwage_search_filter_scores if host_form else lib().kwage_search_filter_scores_device
        return fn(group._h, fset._h, ptr, row_elems, 0, None)
    try:
        p = out.data_ptr()
        assert p % 16 == 0
        for what, group, fset, ptr, row_elems, code in (("row_elems below the span", ga, fs, p, span - 4, -1),
                                                        ("row_elems not a multiple of 4", ga, fs, p, span + 2, -1),
                                                        ("misaligned pointer", ga, fs, p + 4, span, -1),
                                                        ("misaligned pointer", ga, fs, p + 8, span + 8, -1),
                                                        ("no matrix", ga, fs, None, span, -1),
                                                        ("mixed contexts", ga, foreign, p, span, -1),
                                                        ("a sparse group", sparse, fs, p, sparse.column_span, -1),
                                                        ("before finalize", unfinished, fs, p, unfinished.column_span, -6)):
            assert call(group, fset, ptr, row_elems) == code, what
            assert lib().kwage_last_error(), what
            assert (out.cpu().numpy() == SENTINEL).all(), what
        for what, group, fset, row_elems, code in (("row_elems below the span", ga, fs, span - 4, -1), ("row_elems not a multiple of 4", ga, fs, span + 2, -1),
                                                   ("mixed contexts", ga, foreign, span, -1), ("before finalize", unfinished, fs, unfinished.column_span, -6)):
            assert call(group, fset, host.ctypes.data, row_elems, host_form=True) == code, what
            assert (host == SENTINEL).all(), what
        for bad in (sparse, unfinished):
            with pytest.raises(ka.KwageError):
                bad.column_bits()
        # an empty set writes nothing; a valid call on the same buffer afterwards, rows span + 8 apart
        empty = ka.FilterSet.from_columns(ga, [])
        assert call(ga, empty, p, span) == 0 and (out.cpu().numpy() == SENTINEL).all()
        assert lib().kwage_search_filter_kernel() == b""
        empty.close()
        view = out[:n * (span + 8)].view(n, span + 8)[:, :span]
        ka.search_filter_scores_device(ga, fs, view)
        assert np.array_equal(view.cpu().numpy().view(np.uint32), expected(pair["ca"][:, pair["cols"]].T, pair["ca"]))
        assert (out[:n * (span + 8)].view(n, span + 8)[:, span:].cpu().numpy() == SENTINEL).all()
    finally:
        foreign.close()
        other_ctx.close()
        unfinished.close()
        sparse.close()


def test_an_empty_filter_gives_a_row_of_zeros(ka, ctx, pair):
    ga = pair["ga"]
    rng = np.random.default_rng(77)
    f01 = np.stack([np.ones(512, dtype=bool), np.zeros(512, dtype=bool), rng.random(512) < 0.5])
    fs = ka.FilterSet.from_bits(ctx, 21, 2, 9, pack_filters(f01))
    try:
        res = ka.search_filter_scores(ga, fs)
        assert np.array_equal(res.scores, expected(f01, pair["ca"])) and not res.scores[1].any()
        assert np.array_equal(res.scores[0], ga.column_bits())                 # the full filter counts every column's bits
    finally:
        fs.close()


def test_reads_to_bits_to_column_and_filter(ka, ctx):
    """Reads -> kwage_bloom_bits_from_batch -> the bits as one column of a group and as a filter set."""
    from kwage_amd import native
    rng = np.random.default_rng(12)
    k, nh, L = 25, 2, 16
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [acgt[rng.integers(0, 4, size=150)].tobytes().decode() for _ in range(60)]
    prm = native.Params(k, nh, L, 0)
    bits = np.zeros((1 << L) // 8, dtype=np.uint8)
    nd = C.c_uint64()
    b = ka.Batch(ctx, reads)
    native.check(native.lib().kwage_bloom_bits_from_batch(ctx._h, C.byref(prm), b._h, bits.ctypes.data, C.byref(nd)))
    b.close()
    set_rows = np.unpackbits(bits, bitorder="little").astype(bool)
    assert 0 < set_rows.sum() <= nh * nd.value
    # a group of three columns: noise, the sample, noise
    img01 = rng.random((1 << L, 3)) < 0.3
    img01[:, 1] = set_rows
    g = ka.Group(ctx, k, nh, L, 128)
    first = g.add_columns(np.packbits(img01, axis=1, bitorder="little"), 3)
    g.finalize()
    fs = ka.FilterSet.from_bits(ctx, k, nh, L, bits[None, :])
    try:
        res = ka.search_filter_scores(g, fs)
        n_bits = int(set_rows.sum())
        assert fs.bit_counts().tolist() == [n_bits] and res.scores[0, first + 1] == n_bits == g.column_bits()[first + 1]
        assert np.array_equal(res.scores[0, first:first + 3], (img01 & set_rows[:, None]).sum(axis=0))
    finally:
        fs.close()
        g.close()


def test_database_similar_matches_numpy(ka, ctx, pair):
    ga, gb, gc, fs, cols = pair["ga"], pair["gb"], pair["gc"], pair["fs"], pair["cols"]
    db = ka.Database([ga, gc, gb])                       # (the middle group has other parameters: left out)
    f01 = pair["ca"][:, cols].T
    shared = np.concatenate([expected(f01, pair["ca"]), expected(f01, pair["cb"])], axis=1).astype(np.int64)
    col_bits = np.concatenate([pair["ca"].sum(axis=0), pair["cb"].sum(axis=0)]).astype(np.int64)
    real = np.concatenate([pair["ra"], pair["rb"]])
    f_bits = f01.sum(axis=1).astype(np.int64)
    sa = ga.column_span
    for k in (1, 7, 10000):
        got = db.similar(fs, k)
        assert len(got) == len(cols)
        for i in range(len(cols)):
            union = f_bits[i] + col_bits - shared[i]
            jac = np.where(union > 0, shared[i].astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)
            order = [c for c in np.argsort(-jac, kind="stable") if real[c]][:k]          # (Jaccard descending, global column ascending)
            exp = [((0, c) if c < sa else (2, c - sa)) + (int(shared[i, c]), int(f_bits[i]), int(col_bits[c]), float(jac[c])) for c in order]
            assert got[i] == exp, (k, i, got[i][:3], exp[:3])
        # the query sample itself: Jaccard 1, first unless an identical column precedes it
        assert all(lst[0][5] == 1.0 for lst in got)
    assert got[1][0][:2] == (0, cols[0]) and got[1][1][:2] == (0, cols[1])              # columns 1 and 2 of A are duplicates: the tie goes to the lower
