"""A copy between two groups whose matrices are both larger than 4 GiB (2^20 rows of 6 KiB and of 4.5 KiB): most rows start
beyond byte 2^32 of either matrix, so the kernel's source and destination offsets are exercised in 64 bits on the device.
The source's columns are random, generated on the device; 300 scattered ones are copied behind a 37-column insert (a
bit-offset tail), and rows 0, 1, the last ones and 64 seeded random rows above byte 2^32 of both matrices are compared
with numpy's extraction from the source rows that Group.read_rows fetches.  Skipped by test_gpu_large_offsets.py's rule:
32 GiB of free HBM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
L, SRC_STRIDE, DST_STRIDE = 20, 6144, 4608


def test_two_groups_above_four_gib():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    ctx = ka.Context(0)
    src = dst = None
    try:
        free, _ = ctx.mem_info()
        if free < 32 * GIB:
            pytest.skip("needs 32 GiB of free HBM")
        nrows = 1 << L
        src = ka.Group(ctx, 31, 2, L, 8 * SRC_STRIDE)
        dst = ka.Group(ctx, 31, 2, L, 8 * DST_STRIDE)
        assert src.device_bytes == nrows * SRC_STRIDE == 6 * GIB and dst.device_bytes == nrows * DST_STRIDE > 4 * GIB
        assert src.add_random_columns(8 * SRC_STRIDE - 128, 99, 64) == 0
        rng = np.random.default_rng(4100)
        head = rng.integers(0, 256, size=(37, nrows // 8), dtype=np.uint8)
        assert dst.insert_filters(head) == 0
        cols = rng.choice(8 * SRC_STRIDE - 128, size=300, replace=False)
        cols[:40] = np.arange(20000, 20040)                       # one run longer than a word among the scattered ones
        assert np.unique(cols).size == 300
        first, st = dst.copy_columns_from(src, cols, timing=True)
        units = (37 + 300 + 127) // 128
        assert first == 37 and st["columns"] == 300 and st["first_unit"] == 0 and st["units"] == units == 3
        assert st["bytes_written"] == nrows * units * 16 and st["kernel_ms"] > 0
        assert (dst.column_span, dst.num_columns, dst.row_bytes) == (344, 337, 43)
        low = (1 << 32) // DST_STRIDE + 1                          # rows from here on start beyond byte 2^32 of BOTH matrices
        rows = np.array(sorted({0, 1, nrows - 2, nrows - 1} | set((low + rng.choice(nrows - low, size=64, replace=False)).tolist())), dtype=np.int64)
        assert int(rows[4]) * DST_STRIDE > 1 << 32 and int(rows[4]) * SRC_STRIDE > 1 << 32
        got = dst.read_rows(rows)
        bits = np.unpackbits(src.read_rows(rows), axis=1, bitorder="little")[:, cols]
        head_bits = np.unpackbits(head[:, rows // 8], axis=1, bitorder="little").reshape(37, rows.size, 8)[:, np.arange(rows.size), rows % 8].T
        want = np.packbits(np.concatenate([head_bits, bits, np.zeros((rows.size, 7), dtype=np.uint8)], axis=1), axis=1, bitorder="little")
        assert bits.any() and not bits.all()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    finally:
        for g in (src, dst):
            if g is not None:
                g.close()
        ctx.close()
