#!/usr/bin/env python3
"""The fold (kwage_group_fold) measured beside its yardsticks, on one box in one process, on compact_bench.py's group
(2^L rows, 8192 random columns, rows 1 KiB apart), for f = 1, 2, 3 and 5 halvings.  The source is not changed by a fold,
so one group serves every case; each case is run --repeat times and every run's kernel time is shown.

Per case: the kernel's HIP-event time (kwage_fold_stats.kernel_ms) with bytes in + out per second (bytes_read +
bytes_written of the same stats: every source byte once, every destination byte once) -- and, in the same process,

  1. kwage_stream_read_gbps of the source matrix: what the box streams from it;
  2. for the first case, the wall time of what a user could do before the fold existed: export_filters of all columns
     (in blocks of --block columns), the OR of every filter's 2^f pieces on the host, insert_filters into a fresh group at
     the short length -- against the wall time of the fold call.

    python tools/fold_bench.py [--log2 23] [--repeat 3] [--block 1024] [--no-alternative]"""
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
ap.add_argument("--block", type=int, default=1024)
ap.add_argument("--no-alternative", action="store_true", help="leave out yardstick 2: nothing crosses to the host")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
FOLDS = [f for f in (1, 2, 3, 5) if f <= L]

with ka.Context(0) as ctx:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
    warm = ka.Group(ctx, K, NH, 10, CAP)          # (a kernel's first launch loads its code object: not timed)
    warm.add_random_columns(CAP, 1, 16)
    for f in FOLDS:
        warm.fold(10 - f)[0].close()
    warm.close()
    g = ka.Group(ctx, K, NH, L, CAP)
    try:
        assert g.add_random_columns(CAP, 7, 16) == 0
        g.finalize()
        print("group: 2^%d rows, %d random columns at density 1/16 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
        for i, f in enumerate(FOLDS):
            L2 = L - f
            stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
            ms, walls = [], []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                h, st = g.fold(L2, timing=True)
                walls.append(time.perf_counter() - t0)
                ms.append(st["kernel_ms"])
                h.close()
            moved = st["bytes_read"] + st["bytes_written"]
            print("fold f=%d  2^%d -> 2^%d rows  units/row %d  kernel ms %s  in %.3f GB + out %.3f GB -> %.0f GB/s (best of %d);  kwage_stream_read_gbps %.0f GB/s;  in+out rate / stream rate %.2f"
                  % (f, L, L2, st["units_per_row"], " ".join("%.3f" % x for x in ms), st["bytes_read"] / 1e9, st["bytes_written"] / 1e9, moved / min(ms) / 1e6,
                     args.repeat, stream, moved / min(ms) / 1e6 / stream))
            if i == 0 and not args.no_alternative:
                t0 = time.perf_counter()
                alt = ka.Group(ctx, K, NH, L2, CAP)
                t_export = t_or = t_insert = 0.0
                for first in range(0, CAP, args.block):
                    t1 = time.perf_counter()
                    long = g.export_filters(list(range(first, min(first + args.block, CAP))))
                    t2 = time.perf_counter()
                    short = np.bitwise_or.reduce(long.reshape(long.shape[0], 1 << f, -1), axis=1)
                    t3 = time.perf_counter()
                    assert alt.insert_filters(short) == first
                    t4 = time.perf_counter()
                    t_export, t_or, t_insert = t_export + t2 - t1, t_or + t3 - t2, t_insert + t4 - t3
                alt.finalize()
                t_alt = time.perf_counter() - t0
                h, _ = g.fold(L2)
                rows = np.random.default_rng(1).choice(1 << L2, size=256, replace=False)
                assert np.array_equal(h.read_rows(rows), alt.read_rows(rows))
                h.close()
                alt.close()
                print("        wall: export %.2f s + host OR %.2f s + insert %.2f s, in all %.2f s; the fold call %.4f s (%.0f x)"
                      % (t_export, t_or, t_insert, t_alt, min(walls), t_alt / min(walls)))
            else:
                print("        wall: the fold call %.4f s" % min(walls))
    finally:
        g.close()
