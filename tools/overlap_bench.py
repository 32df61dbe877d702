#!/usr/bin/env python3
"""The overlap matrix (kwage_group_column_overlaps) measured beside its yardstick, on one box in one process, on
compact_bench.py's group (2^L rows, 8192 random columns at density 1/4, rows 1 KiB apart).  Both sides are only read, so
one group serves every case; each case is run --repeat times after one untimed call and every run's kernel time is shown.

  a. symmetric, all 8192 columns
  b. 256 listed scattered columns against all columns
  c. 128 x 128 columns (two aligned ranges)
  d. case a on the group folded to 2^(L - 2) rows

Per case: the kernels' HIP-event time (kwage_overlap_stats.kernel_ms), the integer operations per second -- 2 * cells
computed * rows, the cells of the tiles that are computed, so half the matrix in the symmetric form --, the bytes the
staging requests per second -- per tile, part and row one dword per straight block and per distinct dword of a gathered
block: what the lanes ask for, whatever the caches serve --, and, in the same process,

  1. kwage_stream_read_gbps of the matrix: what the box streams from it, taken beside each case;
  2. the yardstick: the same cells through FilterSet.from_columns + search_filter_scores_device on the same group -- the
     only way to them before.  It reads every row a filter has set, whole, for every filter: on at most --yardstick
     filters of the case's a-side (case a: always a chunk) and scaled to the case's filter count; the line says which.

    python tools/overlap_bench.py [--log2 23] [--repeat 3] [--yardstick 64]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (a one-shot program: no second candidate block for the matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=23)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--yardstick", type=int, default=64, help="most filters the filter search is timed on (0: leave the yardstick out)")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
rng = np.random.default_rng(14)

CASES = [("a. symmetric, all 8192 columns", None, False, None),
         ("b. 256 scattered columns against all", np.sort(rng.choice(CAP, size=256, replace=False)), True, None),
         ("c. 128 x 128 columns", np.arange(1024, 1152), True, np.arange(4096, 4224))]


def requested_bytes(cols, span, tiles_other):
    """Bytes one pass over a list's blocks asks for per row, times the tiles of the other side that stage it again."""
    if cols is None:
        return 4 * ((span + 31) // 32) * tiles_other
    n = 0
    for i in range(0, len(cols), 32):
        n += len(np.unique(np.asarray(cols[i:i + 32]) // 32))
    return 4 * n * tiles_other


def run_case(ctx, g, what, cols_a, with_b, cols_b):
    import torch
    nrows = 1 << int(g.params.log_2_filter_len)
    span = g.column_span
    n_a = span if cols_a is None else len(cols_a)
    n_b = n_a if not with_b else span if cols_b is None else len(cols_b)
    out = torch.empty((n_a, n_b), dtype=torch.int32, device="cuda")
    stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
    other = g if with_b else None
    g.column_overlaps(cols_a, other, cols_b, out=out)             # (untimed: the first launch loads the code object)
    ms = []
    for _ in range(args.repeat):
        _, st = g.column_overlaps(cols_a, other, cols_b, out=out, timing=True)
        ms.append(st["kernel_ms"])
    ta, tb = (n_a + 127) // 128, (n_b + 127) // 128
    ops = 2.0 * st["tiles"] * 128 * 128 * nrows
    if with_b:
        req = nrows * (requested_bytes(cols_a, span, tb) + requested_bytes(cols_b, span, ta))
    else:                                                          # (tile index t is the a side of ta - t tiles and the b side of t + 1)
        req = nrows * requested_bytes(cols_a, span, ta + 1)
    best = min(ms)
    print("overlap %-38s cells %d x %d  tiles=%d splits=%d straight=%d gathered=%d  %s  kernel ms %s  %.3e integer ops -> %.1f Tops/s (best of %d);  "
          "requested %.1f GB -> %.0f GB/s;  kwage_stream_read_gbps %.0f GB/s"
          % (what, n_a, n_b, st["tiles"], st["splits"], st["straight_blocks"], st["gathered_blocks"], st["kernel"], " ".join("%.3f" % x for x in ms),
             ops, ops / best / 1e9, args.repeat, req / 1e9, req / best / 1e6, stream), flush=True)
    if args.yardstick > 0:
        fa = np.flatnonzero(g.real_columns()) if cols_a is None else np.asarray(cols_a)
        chunk = fa[:min(len(fa), args.yardstick)]
        t0 = time.perf_counter()
        fs = ka.FilterSet.from_columns(g, chunk)
        t_set = time.perf_counter() - t0
        try:
            scores = torch.empty((len(chunk), (span + 3) // 4 * 4), dtype=torch.int32, device="cuda")
            r = ka.search_filter_scores_device(g, fs, scores, flags=2)
        finally:
            fs.close()
        side_b = cols_b if with_b else cols_a
        tb_cols = torch.from_numpy(np.arange(span) if side_b is None else np.asarray(side_b)).cuda()
        mine = out[torch.from_numpy(chunk).cuda()] if cols_a is None else out[:len(chunk)]
        same = bool((scores[:, tb_cols] == mine).all().item())
        scale = len(fa) / len(chunk)
        print("        yardstick: FilterSet.from_columns of %d filters %.2f s + filter search kernels %.1f ms (%s)%s -> %.1f ms for the case's %d filters; "
              "same cells: %s;  the filter search / the overlap kernels: %.1f x"
              % (len(chunk), t_set, r.kernel_ms, r.kernel, "" if scale == 1 else ", scaled by %.0f" % scale, r.kernel_ms * scale, len(fa), same,
                 r.kernel_ms * scale / best), flush=True)


with ka.Context(0) as ctx:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
    warm = ka.Group(ctx, K, NH, 10, CAP)              # (a kernel's first launch loads its code object: not timed)
    warm.add_random_columns(CAP, 1, 64)
    warm.finalize()
    warm.column_overlaps_host([0, 1])
    warm.close()
    g = ka.Group(ctx, K, NH, L, CAP)
    folded = None
    try:
        assert g.add_random_columns(CAP, 7, 64) == 0
        g.finalize()
        print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9), flush=True)
        for what, cols_a, with_b, cols_b in CASES:
            run_case(ctx, g, what, cols_a, with_b, cols_b)
        folded, _ = g.fold(L - 2)
        print("group folded to 2^%d rows (%.2f GB resident)" % (L - 2, folded.device_bytes / 1e9), flush=True)
        run_case(ctx, folded, "d. symmetric, all 8192 columns, folded", None, False, None)
    finally:
        if folded is not None:
            folded.close()
        g.close()
