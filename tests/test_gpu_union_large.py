"""A union within one group whose matrix is larger than 4 GiB (2^20 rows of 6 KiB): most rows start beyond byte 2^32, so the
kernel's source and destination offsets are exercised in 64 bits on the device.  The columns are random, generated on the
device; sets of three scattered members are united behind them in the same group (dst == src), and rows 0, 1, the last
ones and 64 seeded random rows above byte 2^32 are compared with numpy's OR over the rows that Group.read_rows fetches.
Correctness only.  Skipped by test_gpu_large_offsets.py's rule: 32 GiB of free HBM."""
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
        rng = np.random.default_rng(4200)
        sets = [[int(c) for c in rng.choice(n_random, size=3, replace=False)] for _ in range(4)] + [[0, n_random - 1, 20000]]
        first, st = g.union_columns(sets, timing=True)
        assert first == n_random and first % 128 == 0 and (st["sets"], st["members"], st["entries"]) == (5, 15, 15)
        assert (st["first_unit"], st["units"], st["bytes_written"]) == (first // 128, 1, nrows * 16) and st["kernel_ms"] > 0
        assert (g.column_span, g.num_columns, g.row_bytes) == (n_random + 8, n_random + 5, n_random // 8 + 1)
        low = (1 << 32) // STRIDE + 1                              # rows from here on start beyond byte 2^32
        rows = np.array(sorted({0, 1, nrows - 2, nrows - 1} | set((low + rng.choice(nrows - low, size=64, replace=False)).tolist())), dtype=np.int64)
        assert int(rows[4]) * STRIDE > 1 << 32
        bits = np.unpackbits(g.read_rows(rows), axis=1, bitorder="little")
        want = np.stack([bits[:, s].any(axis=1) for s in sets], axis=1)
        assert want.any() and not want.all()
        assert np.array_equal(bits[:, first:first + 5], want), np.argwhere(bits[:, first:first + 5] != want)[:5]
        assert not bits[:, first + 5:].any()
    finally:
        if g is not None:
            g.close()
        ctx.close()
