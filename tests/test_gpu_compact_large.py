"""Compaction of one 6 GiB group (2^20 rows of 6 KiB): two thirds of its rows start beyond byte 2^32 of the matrix, so the
kernel's row offsets, loads and stores are exercised in 64 bits on the device.  Sampled rows -- the first, the last, the
ones around byte 2^32 and 4096 random ones -- are read before the call, packed by the numpy reference
(tests/compact_cases.py) and compared with the same rows read after it.  Skipped by test_gpu_large_offsets.py's rule: 32 GiB
of free HBM."""
import numpy as np
import pytest

import compact_cases as cc
import large_shapes as ls

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
        assert g.add_random_columns(cap - 128, 97, 64) == 0
        g.finalize()
        span = g.column_span
        assert span == cap - 128
        # a shift of one bit from the start, holes across word and unit boundaries, a whole unit, and the last column
        gone = sorted({0, 31, 32, 127, 128, 129, 40000, span - 1} | set(range(20096, 20096 + 128)) | set(range(30001, 30200, 2)))
        g.retire_columns(gone)
        valid = np.ones(span, dtype=bool)
        valid[gone] = False
        rng = np.random.default_rng(3000)
        rows = np.array(sorted(set(ls.rows_around(nrows, STRIDE)) | set(rng.choice(nrows, size=4096, replace=False).tolist())))
        assert rows[-1] == nrows - 1 and int(rows[-1]) * STRIDE > 1 << 32
        before = np.unpackbits(g.read_rows(rows), axis=1, bitorder="little").astype(bool)
        assert before[:, valid].any() and not before[:, gone].any()
        want = cc.reference(before, valid)
        new, st = g.compact(timing=True)
        m = int(valid.sum())
        assert st["columns"] == m == g.num_columns and st["span_before"] == span and st["span_after"] == (m + 7) // 8 * 8 == g.column_span
        assert st["first_unit"] == 0 and st["units"] == span // 128 and st["kernel_ms"] > 0
        assert st["runs"] == int(1 + np.count_nonzero(np.diff(np.flatnonzero(valid)) != 1))
        assert np.array_equal(new, np.where(valid, np.cumsum(valid) - 1, -1))
        got = g.read_rows(rows)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    finally:
        if g is not None:
            g.close()
        ctx.close()
