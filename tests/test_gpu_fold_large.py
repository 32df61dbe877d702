"""The fold of one 6 GiB group (2^20 rows of 6 KiB) to 2^19 and to 2^17 rows: two thirds of the source's rows start beyond
byte 2^32 of its matrix, so the kernel's source offsets are exercised in 64 bits on the device.  Destination rows 0, 1,
the last one and 64 seeded random ones are compared with numpy's OR of the source rows that fall on them, which
Group.read_rows fetches.  Skipped by test_gpu_large_offsets.py's rule: 32 GiB of free HBM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
L, STRIDE = 20, 6144


def test_six_gib_group():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    ctx = ka.Context(0)
    g = None
    try:
        free, _ = ctx.mem_info()
        if free < 32 * GIB:
            pytest.skip("needs 32 GiB of free HBM")
        nrows, cap = 1 << L, 8 * STRIDE
        g = ka.Group(ctx, 31, 2, L, cap)
        assert g.row_stride == STRIDE and g.device_bytes == nrows * STRIDE == 6 * GIB
        assert g.add_random_columns(cap - 128, 98, 16) == 0          # density 1/16: eight rows ORed stay far from full
        g.finalize()
        rb = g.row_bytes
        assert rb == STRIDE - 16
        for L2 in (19, 17):
            f, st = g.fold(L2, timing=True)
            try:
                n2, fold = 1 << L2, 1 << (L - L2)
                units = (rb + 15) // 16
                assert st["units_per_row"] == units == 383 and st["bytes_written"] == n2 * units * 16 and st["bytes_read"] == nrows * units * 16
                assert st["bytes_read"] >= 1 << 32 and st["kernel_ms"] > 0
                assert (f.row_bytes, f.column_span, f.num_columns, f.row_stride, f.device_bytes) == (rb, g.column_span, g.num_columns, STRIDE, n2 * STRIDE)
                rng = np.random.default_rng(3100 + L2)
                rows = np.array(sorted({0, 1, n2 - 1} | set(rng.choice(n2, size=64, replace=False).tolist())), dtype=np.int64)
                src_rows = (rows[:, None] + n2 * np.arange(fold, dtype=np.int64)[None, :]).reshape(-1)
                assert src_rows.max() == nrows - 1 and int(src_rows.max()) * STRIDE > 1 << 32
                src = g.read_rows(src_rows).reshape(rows.size, fold, rb)
                want = np.bitwise_or.reduce(src, axis=1)
                assert want.any() and not want.all()
                got = f.read_rows(rows)
                assert np.array_equal(got, want), np.argwhere(got != want)[:5]
            finally:
                f.close()
    finally:
        if g is not None:
            g.close()
        ctx.close()
