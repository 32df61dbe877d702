"""kwage_search_presence / kwage_search_presence_device (the presence search) through the C ABI and the Python mirror.

Expected bitmap: bit (q, c) is set exactly where the CPU oracle (oracle.search_image at the same threshold) lists column
c for query q; 0 on pad bits and for queries without k-mers.  Every comparison is exact equality of bits.  The device's
own threshold search (kwage_search at t = 0.5 and 1) is a second oracle.

(The contract's last argument errors -- a query of 2^32 rows and more, a batch too large for one launch -- need queries
of 859 M bases at five hash functions or 2^32 (query, tile) pairs: like the same checks of the score search they are not
exercised here.)"""
import numpy as np
import pytest

import presence_shapes as ps
from test_gpu_scores import make_group, the_queries

pytestmark = pytest.mark.gpu

FLOOR_ZERO = 1e-12
THRESHOLDS = (FLOOR_ZERO, 0.5, 0.8, 1.0)
FILES_NF = [3001, 8667]
DUP_PAIRS = [(3, 4), (3, 900), (17, 2000), (100, 101), (5000, 5001)]


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


def written(g):
    return (g.row_bytes + 15) // 16 * 16


def real_columns(files, span):
    real = np.zeros(span, dtype=bool)
    for first, _, nf in files:
        real[first:first + nf] = True
    return real


def oracle_bitmap(oracle, files, span, k, num_hash, L, queries, threshold):
    """(bool [n, span] expected bitmap, n per query): the oracle's hits at float32(threshold), scattered."""
    exp = np.zeros((len(queries), span), dtype=bool)
    nk = []
    for q, seq in enumerate(queries):
        kmers = oracle.unique_kmers(seq, k)
        nk.append(len(kmers))
        if not len(kmers):
            continue
        for first, img, nf in files:
            hits, _ = oracle.search_image(img, img.shape[1], k, num_hash, L, nf, kmers, float(np.float32(threshold)))
            exp[q, [first + c for c, _ in hits]] = True
    return exp, np.asarray(nk, dtype=np.uint32)


def popcounts(bits):
    return np.unpackbits(np.ascontiguousarray(bits), axis=1).sum(axis=1).astype(np.uint32)


def expected_kernel(segs, t, num_hash, positions):
    if segs == 1:
        return ps.AND_NAME if t == 1.0 else ps.tile_name(20, num_hash)
    if segs == 3:
        return ps.combine_name(20, num_hash, positions)
    return None


@pytest.mark.parametrize("num_hash", [1, 3, 5])
def test_presence_matches_oracle(ka, ctx, oracle, num_hash):
    rng = np.random.default_rng(170 + num_hash)
    kmer, L = 21, 11
    density = {1: 0.35, 3: 0.7, 5: 0.82}[num_hash]
    g, files = make_group(ka, ctx, rng, kmer, num_hash, L, FILES_NF, density, DUP_PAIRS, full_cols=(11, 8600))
    _, queries = the_queries(rng)
    span = g.column_span
    assert span > 8192 and span % 8 == 0 and span < g.row_stride * 8          # two tiles, the last one cut by the span
    real = real_columns(files, span)
    b = ka.Batch(ctx, queries)
    try:
        for t in THRESHOLDS:
            exp, nk = oracle_bitmap(oracle, files, span, kmer, num_hash, L, queries, t)
            assert nk[5] == 0 and nk[6] == 0 and nk[7] > 90000
            assert all(exp[q, files[1][0] + 8600] for q in np.flatnonzero(nk))    # the all-ones columns pass at every threshold
            if t == FLOOR_ZERO:
                assert all(np.array_equal(exp[q], real) for q in np.flatnonzero(nk))     # floor 0: every real column
            # default: this small batch (fewer than 2048 tiles) takes the segmented form; force_segs=1: one wave per
            # (query, 8192-column tile) -- the AND kernel at t = 1
            for segs in (0, 1, 3):
                pair = []
                for flags in (ka.SEARCH_TIMING, ka.SEARCH_TIMING | ka.SEARCH_EARLY_EXIT):
                    with ctx.tuning(force_segs=segs):
                        res = ka.search_presence(g, b, t, flags)
                    name = expected_kernel(segs, t, num_hash, int(nk[7]))
                    if name is None:
                        assert res.kernel.startswith("count_kernel<") and res.kernel.endswith("+presence_combine_kernel<20>"), res.kernel
                    else:
                        assert res.kernel == name, (segs, t, res.kernel, name)
                    assert res.bits.dtype == np.uint8 and res.bits.shape == (len(queries), g.row_bytes)
                    assert np.array_equal(res.num_query_kmer, nk), (t, segs, flags)
                    got = res.unpack()
                    assert got.dtype == bool and got.shape == exp.shape
                    bad = np.argwhere(got != exp)
                    assert bad.size == 0, (num_hash, t, segs, flags, res.kernel, bad[:5].tolist())
                    assert not got[:, ~real].any() and not got[nk == 0].any()             # pad bits, queries without k-mers
                    assert np.array_equal(res.passing, popcounts(res.bits)) and np.array_equal(res.passing, exp.sum(axis=1))
                    assert res.kernel_ms > 0
                    pair.append(np.array(res.bits))
                assert np.array_equal(pair[0], pair[1]), (t, segs)                       # with and without the early exit
    finally:
        b.close()
        g.close()


@pytest.fixture(scope="module")
def small(ka, ctx, oracle):
    """One group (two files, 11.7 k columns, 2^11 rows, three hash functions), its queries (the long one 3000 bases)
    and the oracle's bitmaps at 0.5 and 1."""
    rng = np.random.default_rng(15)
    kmer, nh, L = 21, 3, 11
    g, files = make_group(ka, ctx, rng, kmer, nh, L, FILES_NF, 0.7, [(3, 4), (17, 2000), (2998, 8000)], full_cols=(7, 2500))
    genome, queries = the_queries(rng, 3000)
    b = ka.Batch(ctx, queries)
    span = g.column_span
    exp = {t: oracle_bitmap(oracle, files, span, kmer, nh, L, queries, t)[0] for t in (0.5, 1.0)}
    nk = oracle_bitmap(oracle, files[:0], span, kmer, nh, L, queries, 0.5)[1]
    yield dict(g=g, files=files, b=b, queries=queries, exp=exp, nk=nk, real=real_columns(files, span), kmer=kmer, nh=nh, L=L, rng=rng)
    b.close()
    g.close()


def unpack(rows, span):
    return np.unpackbits(np.ascontiguousarray(rows), axis=1, bitorder="little")[:, :span].astype(bool)


def test_floors_are_kwage_query_thresholds(ka, ctx, oracle):
    """Row q is `count >= kwage_query_threshold(t, n)` on the real columns; at (t, n) = (0.7, 100) -- a pair at which the
    float32 product truncates to 70 and a double product to 69 -- a column with 70 matches passes, one with 69 does not."""
    from kwage_amd.native import lib
    rng = np.random.default_rng(99)
    kmer, nh, L, nf = 21, 3, 11, 300
    probe = "".join(rng.choice(list("ACGT"), size=120))
    kmers = oracle.unique_kmers(probe, kmer)
    bits = rng.random((1 << L, nf)) < 0.7
    rows = oracle.row_indices(kmers, kmer, nh, L)
    for col, cnt in ((40, 69), (41, 70)):
        bits[:, col] = False
        bits[rows[:cnt].reshape(-1), col] = True
    img = np.packbits(bits, axis=1, bitorder="little")
    _, more = the_queries(rng, 3000)
    queries = [probe] + more
    g = ka.Group(ctx, kmer, nh, L, nf + 128)
    first = g.add_columns(img, nf)
    g.finalize()
    b = ka.Batch(ctx, queries)
    try:
        span = g.column_span
        counts = np.zeros((len(queries), span), dtype=np.int64)
        nk = []
        for q, seq in enumerate(queries):
            km = oracle.unique_kmers(seq, kmer)
            nk.append(len(km))
            if len(km):
                for c, m in oracle.search_image(img, img.shape[1], kmer, nh, L, nf, km, FLOOR_ZERO)[0]:
                    counts[q, first + c] = m
        assert nk[0] == 100 and counts[0, first + 40] == 69 and counts[0, first + 41] == 70
        assert lib().kwage_query_threshold(0.7, 100) == 70 and int(float(np.float32(0.7)) * 100) == 69
        real = np.zeros(span, dtype=bool)
        real[first:first + nf] = True
        for t in (0.7, 0.5, 0.9, 1.0, FLOOR_ZERO):
            floors = np.array([lib().kwage_query_threshold(float(t), n) for n in nk], dtype=np.int64)
            if t == 1.0:
                assert floors.tolist() == nk
            exp = (counts >= floors[:, None]) & real[None, :] & (np.array(nk) > 0)[:, None]
            for segs in (1, 3):
                with ctx.tuning(force_segs=segs):
                    res = ka.search_presence(g, b, t)
                assert np.array_equal(res.unpack(), exp), (t, segs, res.kernel)
            if t == 0.7:
                assert exp[0, first + 41] and not exp[0, first + 40]
    finally:
        b.close()
        g.close()


def test_presence_agrees_with_the_threshold_search(ka, ctx, small):
    g, b, nk = small["g"], small["b"], small["nk"]
    for t in (0.5, 1.0):
        thr = g.search(b, t)
        assert np.array_equal(thr.num_query_kmer, nk)
        h = thr.hits
        mine = np.zeros((b.n, g.column_span), dtype=bool)
        mine[h["query"], h["column"]] = True
        assert h.size and np.array_equal(mine, small["exp"][t])
        for segs in (0, 1):
            for flags in (0, ka.SEARCH_EARLY_EXIT):
                with ctx.tuning(force_segs=segs):
                    res = ka.search_presence(g, b, t, flags)
                assert np.array_equal(res.unpack(), mine), (t, segs, flags, res.kernel)
                assert np.array_equal(res.passing, np.bincount(h["query"], minlength=b.n))


def test_bytes_beyond_the_row_are_untouched(ka, ctx, small):
    import torch
    from kwage_amd.native import lib, check
    g, b, nk = small["g"], small["b"], small["nk"]
    n, span, w = b.n, g.column_span, written(g)
    rb = w + 32
    for t in (0.5, 1.0):
        exp = small["exp"][t]
        for segs in (1, 3):
            with ctx.tuning(force_segs=segs):
                # device form: rows 32 bytes longer than what is written, and 64 bytes behind the last row
                flat = torch.full((n * rb + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
                out = flat[:n * rb].view(n, rb)
                pas = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                nkd = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                res = ka.search_presence_device(g, b, t, out, pas, nkd)
                got = flat.cpu().numpy()
                rows = got[:n * rb].reshape(n, rb)
                assert (rows[:, w:] == 0xA5).all() and (got[n * rb:] == 0xA5).all(), (t, segs)
                assert np.array_equal(unpack(rows[:, :w], span), exp), (t, segs, res.kernel)
                assert not rows[:, g.row_bytes:w].any()                                 # the bytes up to W: 0, not the fill
                assert np.array_equal(nkd.cpu().numpy().view(np.uint32), nk)
                assert np.array_equal(pas.cpu().numpy().view(np.uint32), exp.sum(axis=1))
                # host form: the same through kwage_search_presence
                host = np.full(n * rb + 64, 0xA5, dtype=np.uint8)
                hp = np.zeros(n, dtype=np.uint32)
                check(lib().kwage_search_presence(g._h, b._h, float(t), host.ctypes.data, rb, hp.ctypes.data, None, 0, None))
                rows = host[:n * rb].reshape(n, rb)
                assert (rows[:, w:] == 0xA5).all() and (host[n * rb:] == 0xA5).all(), (t, segs)
                assert np.array_equal(unpack(rows[:, :w], span), exp) and np.array_equal(hp, exp.sum(axis=1)), (t, segs)


def test_early_exit_writes_its_zeros(ka, ctx, oracle):
    """A tile in which no column can pass stops early and must still store its zeros: the output is pre-filled with
    0xFF.  Tile 0 (columns 0 ... 8191) holds sparse random columns only, tile 1 an all-ones column."""
    import torch
    rng = np.random.default_rng(123)
    kmer, nh, L = 21, 1, 11
    g, files = make_group(ka, ctx, rng, kmer, nh, L, FILES_NF, 0.3, [], full_cols=(8600,))
    _, queries = the_queries(rng, 3000)
    b = ka.Batch(ctx, queries)
    try:
        n, span, w = b.n, g.column_span, written(g)
        full = files[1][0] + 8600
        assert full >= 8192 and w > 1024
        for t in (1.0, 0.8):
            exp, nk = oracle_bitmap(oracle, files, span, kmer, nh, L, queries, t)
            assert not exp[:, :8192].any() and all(exp[q, full] for q in np.flatnonzero(nk))
            out = torch.full((n, w), 0xFF, dtype=torch.uint8, device="cuda:0")
            with ctx.tuning(force_segs=1):
                res = ka.search_presence_device(g, b, t, out, flags=ka.SEARCH_EARLY_EXIT)
            assert res.kernel == (ps.AND_NAME if t == 1.0 else ps.tile_name(14, nh)), res.kernel
            got = out.cpu().numpy()
            assert not got[:, :1024].any(), t                                           # the tile that stopped
            assert np.array_equal(unpack(got, span), exp), t
            assert not got[nk == 0].any() and all(got[q, full // 8] >> (full % 8) & 1 for q in np.flatnonzero(nk))
    finally:
        b.close()
        g.close()


def test_refusals_leave_the_buffers_untouched(ka, ctx, small):
    import torch
    from kwage_amd.native import lib
    g, b = small["g"], small["b"]
    n, w = b.n, written(g)
    out = torch.full((n * (w + 16) + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    words = torch.full((2 * n,), -7, dtype=torch.int32, device="cuda:0")
    host = np.full(n * (w + 16), 0xA5, dtype=np.uint8)
    hwords = np.full(2 * n, 0xA5A5A5A5, dtype=np.uint32)
    other_ctx = ka.Context(0)
    foreign = ka.Batch(other_ctx, small["queries"])
    unfinished = ka.Group(ctx, small["kmer"], small["nh"], small["L"], 1000)
    unfinished.add_random_columns(1000, 3, 64)

    def call(group, batch, t, ptr, row_bytes, host_form=False):
        if host_form:
            return lib().kwage_search_presence(group._h, batch._h, float(t), ptr, row_bytes, hwords.ctypes.data, hwords[n:].ctypes.data, 0, None)
        return lib().kwage_search_presence_device(group._h, batch._h, float(t), ptr, row_bytes, words.data_ptr(), words[n:].data_ptr(), 0, None)
    try:
        p = out.data_ptr()
        assert p % 16 == 0
        cases = [("row_bytes below W", g, b, 0.5, p, w - 16, -1),
                 ("row_bytes not a multiple of 16", g, b, 0.5, p, w + 8, -1),
                 ("misaligned pointer", g, b, 0.5, p + 4, w, -1),
                 ("misaligned pointer", g, b, 1.0, p + 8, w + 16, -1),
                 ("no bitmap", g, b, 0.5, None, w, -1),
                 ("t below 0", g, b, -0.1, p, w, -1),
                 ("t above 1", g, b, 1.5, p, w, -1),
                 ("t not a number", g, b, float("nan"), p, w, -1),
                 ("mixed contexts", g, foreign, 0.5, p, w, -1),
                 ("before finalize", unfinished, b, 0.5, p, (unfinished.row_bytes + 15) // 16 * 16, -6)]
        for what, group, batch, t, ptr, row_bytes, code in cases:
            assert call(group, batch, t, ptr, row_bytes) == code, what
            assert lib().kwage_last_error(), what
            assert (out.cpu().numpy() == 0xA5).all() and (words.cpu().numpy() == -7).all(), what
        for what, group, batch, t, ptr, row_bytes, code in cases:
            if what in ("misaligned pointer", "no bitmap"):
                continue                                      # (host memory needs no alignment; NULL below)
            assert call(group, batch, t, host.ctypes.data, row_bytes, host_form=True) == code, what
            assert (host == 0xA5).all() and (hwords == 0xA5A5A5A5).all(), what
        assert call(g, b, 0.5, None, w, host_form=True) == -1 and (hwords == 0xA5A5A5A5).all()
        with pytest.raises(ValueError):
            ka.search_presence_device(g, b, 0.5, out[:n * w].view(n, w).to(torch.int32))
        with pytest.raises(ValueError):
            ka.search_presence_device(g, b, 0.5, out[:n * (w - 16)].view(n, w - 16))
        # and a valid call on the same buffer afterwards: rows W + 16 apart
        view = out[:n * (w + 16)].view(n, w + 16)[:, :w]
        ka.search_presence_device(g, b, 0.5, view)
        assert np.array_equal(unpack(view.cpu().numpy(), g.column_span), small["exp"][0.5])
    finally:
        unfinished.close()
        foreign.close()
        other_ctx.close()


def test_sparse_group_gives_the_full_groups_bitmap(ka, ctx, small):
    import torch
    g, b, files = small["g"], small["b"], small["files"]
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
        for t in (0.5, 1.0):
            for segs in (1, 3):
                with ctx.tuning(force_segs=segs):
                    full, part = ka.search_presence(g, b, t), ka.search_presence(sp, b, t)
                assert part.kernel == full.kernel and np.array_equal(part.bits, full.bits)
                assert np.array_equal(full.unpack(), small["exp"][t]) and np.array_equal(part.passing, full.passing)
        # a sparse group made for other queries: refused, nothing written
        w = written(sp)
        out = torch.full((1, w), 0xA5, dtype=torch.uint8, device="cuda:0")
        words = torch.full((2,), -7, dtype=torch.int32, device="cuda:0")
        for t in (0.5, 1.0):
            with pytest.raises(ka.KwageError) as ei:
                ka.search_presence_device(sp, other, t, out, words[:1], words[1:])
            assert ei.value.code == -6 and "not among the rows" in str(ei.value), ei.value
            assert (out.cpu().numpy() == 0xA5).all() and (words.cpu().numpy() == -7).all()
        assert np.array_equal(ka.search_presence(sp, b, 0.5).unpack(), small["exp"][0.5])      # still gives the right bitmap
    finally:
        other.close()
        sp.close()


def test_several_groups_side_by_side(ka, ctx, oracle, small):
    import torch
    g, b, queries = small["g"], small["b"], small["queries"]
    rng = np.random.default_rng(16)
    g2, files2 = make_group(ka, ctx, rng, small["kmer"], 1, 10, [777, 1500], 0.4, [(1, 2)], full_cols=(5,))
    try:
        assert g2.row_bytes % 16 != 0 or g.row_bytes % 16 != 0          # a block that ends inside its last 16 bytes
        for t in (0.5, 1.0):
            both, bases = ka.Database([g2, g]).search_presence(b, t)
            w2, w = written(g2), written(g)
            assert tuple(both.shape) == (b.n, w2 + w) and both.dtype == torch.uint8 and bases == [0, w2 * 8]
            got = both.cpu().numpy()
            one2, one = ka.search_presence(g2, b, t), ka.search_presence(g, b, t)
            exp2, _ = oracle_bitmap(oracle, files2, g2.column_span, small["kmer"], 1, 10, queries, t)
            assert np.array_equal(one2.unpack(), exp2) and np.array_equal(one.unpack(), small["exp"][t])
            assert np.array_equal(got[:, :g2.row_bytes], one2.bits) and np.array_equal(got[:, w2:w2 + g.row_bytes], one.bits)
            assert not got[:, g2.row_bytes:w2].any() and not got[:, w2 + g.row_bytes:].any()      # zeros between the blocks
    finally:
        g2.close()
