"""Export from one 6 GiB group (2^20 rows of 6 KiB): two thirds of its rows start beyond byte 2^32 of the matrix, so the
kernel's row offsets are exercised in 64 bits on the device.  Three columns are exported into a device tensor and compared
with Group.read_rows on rows sampled from the first, the middle and the last 4096 rows.  Skipped by
test_gpu_large_offsets.py's rule: 32 GiB of free HBM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
L, STRIDE = 20, 6144


def test_six_gib_group():
    import torch
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
        g.retire_columns([40000])
        cols = np.array([span - 1, 33, 20001])              # the row's last dword, a bit offset, somewhere in the middle
        rng = np.random.default_rng(3100)
        rows = np.concatenate([np.sort(rng.choice(4096, size=256, replace=False)) + base for base in (0, nrows // 2 - 2048, nrows - 4096)])
        rows = np.unique(np.concatenate([rows, [0, nrows - 1]]))
        assert int(rows[-1]) * STRIDE > 1 << 32
        fb = nrows // 8
        dev = torch.full((3, fb + 64), 0xA5, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
        _, ms = g.export_filters(cols, out=dev[:, :fb], timing=True)
        got = dev.cpu().numpy()
        assert ms > 0 and (got[:, fb:] == 0xA5).all()
        want = np.unpackbits(g.read_rows(rows), axis=1, bitorder="little")[:, cols].astype(bool)          # [rows, 3]
        bits = ((got[:, rows // 8] >> (rows % 8).astype(np.uint8)) & 1).astype(bool)                        # [3, rows]
        assert want.any() and not want.all()
        assert np.array_equal(bits.T, want), np.argwhere(bits.T != want)[:5]
    finally:
        if g is not None:
            g.close()
        ctx.close()
