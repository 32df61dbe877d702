"""Nearest-neighbour lists whose strip of cells is larger than 4 GiB: 1152 listed queries against 2^20 random candidate
columns of 8 rows in ONE strip (the strip budget raised to 4.8 GB), so the cells of every entry from 1024 on lie beyond
byte 2^32 of the strip's block and the select kernel's row offsets are exercised in 64 bits on the device.  16 entries,
ten of them beyond entry 1024, are compared with a model computed for just those entries: at 8 rows a union is at most
16, so shared * lcm(1 .. 16) / union is an exact integer key, sorted with the index by numpy.  Correctness only.  Skipped
below 16 GiB of free HBM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
L, CANDIDATES, QUERIES, K = 3, 1 << 20, 1152, 24
LCM_16 = 720720


def test_a_strip_of_cells_above_four_gib():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    ctx = ka.Context(0)
    g = None
    try:
        free, _ = ctx.mem_info()
        if free < 16 * GIB:
            pytest.skip("needs 16 GiB of free HBM")
        g = ka.Group(ctx, 31, 2, L, CANDIDATES)
        assert g.add_random_columns(CANDIDATES, 77, 96) == 0 and g.column_span == CANDIDATES
        rng = np.random.default_rng(4800)
        queries = rng.choice(CANDIDATES, size=QUERIES, replace=False)
        entries = np.sort(np.concatenate([rng.choice(1024, size=6, replace=False), 1024 + rng.choice(QUERIES - 1024, size=8, replace=False), [1024, QUERIES - 1]]))
        assert len(entries) == 16 and (entries >= 1024).sum() >= 8
        bits = np.unpackbits(g.read_rows(np.arange(1 << L)), axis=1, bitorder="little")[:, :CANDIDATES].astype(np.int64)       # [8, 2^20]
        own = bits.sum(axis=0)
        index = np.arange(CANDIDATES)
        strip_bytes = QUERIES * CANDIDATES * 4
        assert strip_bytes > 4 * GIB and 1024 * CANDIDATES * 4 == 1 << 32
        for metric, skip in (("jaccard", True), ("shared", False)):
            with ctx.tuning(neighbors_strip_bytes=strip_bytes):
                rec, cnt, st = g.column_neighbors(K, queries, g, None, metric=metric, skip_self=skip)
            assert (st["strips"], st["strip_entries"], st["n_b"], st["tiles"]) == (1, QUERIES, CANDIDATES, 9 * (CANDIDATES // 128)), st
            rec, cnt = rec[entries].cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
            assert (cnt == K).all()
            for e, got in zip(entries, rec):
                q = queries[e]
                shared = bits[:, q] @ bits
                union = own[q] + own - shared
                key = shared if metric == "shared" else np.where(union > 0, shared * LCM_16 // np.maximum(union, 1), 0)
                assert metric == "shared" or ((shared * LCM_16) % np.maximum(union, 1) == 0).all()
                order = np.lexsort((index, -key))
                if skip:
                    order = order[order != q]
                top = order[:K]
                want = np.stack([top, shared[top], np.full(K, own[q]), own[top]], axis=1).astype(np.uint32)
                assert np.array_equal(got, want), (e, got[:4], want[:4])
    finally:
        if g is not None:
            g.close()
        ctx.close()
