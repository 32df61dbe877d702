#!/usr/bin/env python3
"""The copy between groups (kwage_group_copy_columns) measured beside its yardsticks, on one box in one process, on
compact_bench.py's group (2^L rows, 8192 random columns, rows 1 KiB apart).  The source is not changed by a copy, so one
group serves every case; each case is run --repeat times into a fresh destination and every run's kernel time is shown.

  a. all columns into a fresh group: the grow (every unit on the aligned fast path, one 16-byte load per unit)
  b. the same behind a one-column insert: every unit shifted by one bit (five source dwords per unit)
  c. every other column: runs of one, every unit walked piece by piece
  d. 128 columns into a wide group: one 16-byte unit of every 1 KiB row

Per case: the kernel's HIP-event time (kwage_copy_stats.kernel_ms) with bytes in + out per second -- in: the distinct
source dwords the list touches, once per row; out: bytes_written of the same stats -- and, in the same process,

  1. kwage_stream_read_gbps of the source matrix: what the box streams from it;
  2. the compaction kernel on the same group with column 0 retired (compact_bench.py's case a: the same read + write
     traffic, in place);
  3. for case a, the wall time of what a user could do before the copy existed: export_filters of all columns (in blocks
     of --block columns) and insert_filters into a fresh group -- against the wall time of the copy call.

    python tools/copy_bench.py [--log2 23] [--repeat 3] [--block 1024] [--no-alternative]"""
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
ap.add_argument("--no-alternative", action="store_true", help="leave out yardstick 3: nothing crosses to the host")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
nrows = 1 << L


def fresh(ctx):
    return ka.Group(ctx, K, NH, L, CAP)


def behind_one(ctx):
    g = ka.Group(ctx, K, NH, L, CAP + 1024)
    assert g.insert_filters(np.zeros((1, max(1, nrows // 8)), dtype=np.uint8)) == 0
    return g


def narrow(ctx):
    return ka.Group(ctx, K, NH, L, CAP // 2)


def wide(ctx):
    g = ka.Group(ctx, K, NH, L, CAP)
    assert g.add_random_columns(CAP // 2, 9, 64) == 0
    return g


CASES = [("a. all columns, fresh group", None, fresh),
         ("b. all columns, behind one column", None, behind_one),
         ("c. every other column", np.arange(0, CAP, 2), narrow),
         ("d. 128 columns into a wide group", np.arange(1000, 1128), wide)]

with ka.Context(0) as ctx:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
    warm, warm2 = ka.Group(ctx, K, NH, 10, CAP), ka.Group(ctx, K, NH, 10, CAP)      # (a kernel's first launch loads its code object: not timed)
    warm.add_random_columns(CAP, 1, 64)
    warm2.copy_columns_from(warm)
    warm.retire_columns([0])
    warm.compact()
    warm.close()
    warm2.close()
    g = fresh(ctx)
    try:
        assert g.add_random_columns(CAP, 7, 64) == 0
        g.finalize()
        print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
        for what, cols, make in CASES:
            stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
            listed = np.arange(CAP) if cols is None else cols
            bytes_in = nrows * 4 * np.unique(listed // 32).size
            ms, walls = [], []
            for _ in range(args.repeat):
                dst = make(ctx)
                try:
                    t0 = time.perf_counter()
                    first, st = dst.copy_columns_from(g, cols, timing=True)
                    walls.append(time.perf_counter() - t0)
                    ms.append(st["kernel_ms"])
                finally:
                    dst.close()
            moved = bytes_in + st["bytes_written"]
            print("copy %-36s n=%5d runs=%4d first=%5d units [%d, %d)  kernel ms %s  in %.3f GB + out %.3f GB -> %.0f GB/s (best of %d);  kwage_stream_read_gbps %.0f GB/s;  in+out rate / stream rate %.2f"
                  % (what, st["columns"], st["runs"], first, st["first_unit"], st["first_unit"] + st["units"], " ".join("%.3f" % x for x in ms),
                     bytes_in / 1e9, st["bytes_written"] / 1e9, moved / min(ms) / 1e6, args.repeat, stream, moved / min(ms) / 1e6 / stream))
            if what.startswith("a") and not args.no_alternative:
                t0 = time.perf_counter()
                alt = fresh(ctx)
                t_export = t_insert = 0.0
                for at in range(0, CAP, args.block):
                    t1 = time.perf_counter()
                    filters = g.export_filters(list(range(at, min(at + args.block, CAP))))
                    t2 = time.perf_counter()
                    assert alt.insert_filters(filters) == at
                    t3 = time.perf_counter()
                    t_export, t_insert = t_export + t2 - t1, t_insert + t3 - t2
                t_alt = time.perf_counter() - t0
                dst = fresh(ctx)
                dst.copy_columns_from(g)
                rows = np.random.default_rng(1).choice(nrows, size=256, replace=False)
                assert np.array_equal(dst.read_rows(rows), alt.read_rows(rows)) and np.array_equal(dst.read_rows(rows), g.read_rows(rows))
                dst.close()
                alt.close()
                print("        wall: export %.2f s + insert %.2f s, in all %.2f s; the copy call %.4f s (%.0f x)" % (t_export, t_insert, t_alt, min(walls), t_alt / min(walls)))
            else:
                print("        wall: the copy call %.4f s" % min(walls))
        # yardstick 2: the compaction kernel on the same group, column 0 retired -- every unit shifted by one bit, in place
        g.retire_columns([0])
        new, cs = g.compact(timing=True)
        bytes_in, bytes_out = nrows * ((CAP - 1 + 7) // 8), nrows * 16 * cs["units"]
        print("compact (column 0 retired, in place)  m=%5d units [%d, %d)  kernel ms %.3f  in %.3f GB + out %.3f GB -> %.0f GB/s"
              % (cs["columns"], cs["first_unit"], cs["first_unit"] + cs["units"], cs["kernel_ms"], bytes_in / 1e9, bytes_out / 1e9, (bytes_in + bytes_out) / cs["kernel_ms"] / 1e6))
    finally:
        g.close()
