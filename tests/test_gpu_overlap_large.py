"""The overlap matrix of a group whose matrix is larger than 4 GiB (2^20 rows of 6 KiB): most rows start beyond byte 2^32,
so the kernel's row offsets are exercised in 64 bits on the device.  The columns are random, generated on the device; 64
listed columns -- a straight block and a gathered one whose members lie in the row's last dwords -- are counted against
each other in the symmetric and the a x b form and compared with the popcounts of the ANDs of the same columns' exported
filters.  Correctness only.  Skipped by test_gpu_large_offsets.py's rule: 32 GiB of free HBM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
L, STRIDE = 20, 6144


def test_one_group_above_four_gib():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    ctx = ka.Context(0)
    g = None
    try:
        free, _ = ctx.mem_info()
        if free < 32 * GIB:
            pytest.skip("needs 32 GiB of free HBM")
        nrows, n_random = 1 << L, 8 * STRIDE - 256
        g = ka.Group(ctx, 31, 2, L, 8 * STRIDE)
        assert g.device_bytes == nrows * STRIDE == 6 * GIB
        assert g.add_random_columns(n_random, 99, 32) == 0
        rng = np.random.default_rng(4300)
        cols = np.concatenate([np.arange(4096, 4128), rng.choice(n_random, size=30, replace=False), [n_random - 1, 0]])
        assert len(cols) == 64
        sym, st = g.column_overlaps_host(cols)
        assert (st["n_a"], st["rows"], st["symmetric"], st["tiles"], st["straight_blocks"], st["gathered_blocks"]) == (64, nrows, 1, 1, 1, 1)
        assert st["splits"] > 1 and (nrows - nrows // st["splits"]) * STRIDE > 1 << 32      # the last part lies wholly beyond byte 2^32
        filters = np.unpackbits(g.export_filters(cols), axis=1, bitorder="little").astype(np.float32)      # [64, 2^20] of 0 / 1: the sums below are exact in float32 blocks
        want = np.zeros((64, 64), dtype=np.int64)
        for r0 in range(0, nrows, 1 << 16):
            block = filters[:, r0:r0 + (1 << 16)]
            want += (block @ block.T).astype(np.int64)
        assert np.array_equal(sym, want) and want.min() > 0
        axb, st = g.column_overlaps_host(cols[:33], g, cols[20:])
        assert st["symmetric"] == 0 and np.array_equal(axb, want[:33, 20:])
    finally:
        if g is not None:
            g.close()
        ctx.close()
