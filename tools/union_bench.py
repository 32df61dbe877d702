#!/usr/bin/env python3
"""The union of columns (kwage_group_union_columns) measured beside its yardsticks, on one box in one process, on
compact_bench.py's group (2^L rows, 8192 random columns, rows 1 KiB apart).  The members are not changed by a union, so
one source group serves every case; each case is run --repeat times into a fresh destination and every run's kernel time
is shown.

  a. one set of 8 scattered members
  b. 2048 sets of 4 consecutive columns (every column of the source once)
  c. 128 sets of 64 scattered members each
  d. one set of all 8192 columns

Per case: the kernel's HIP-event time (kwage_union_stats.kernel_ms) with bytes in + out per second -- in: the distinct
64-byte lines of a source row the lists touch, once per row (a dword load brings its line); out: bytes_written of the same
stats --, the dword loads a lane issues, and, in the same process,

  1. kwage_stream_read_gbps of the source matrix: what the box streams from it, taken beside each case;
  2. the wall time of what a user could do before the union existed: export_filters of the members, numpy's OR,
     insert_filters into a fresh group -- against the wall time of the union call, the results compared on sampled rows.

    python tools/union_bench.py [--log2 23] [--repeat 3] [--no-alternative]"""
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
ap.add_argument("--no-alternative", action="store_true", help="leave out yardstick 2: nothing crosses to the host")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
nrows = 1 << L
rng = np.random.default_rng(13)

CASES = [("a. one set of 8 scattered members", [sorted(int(c) for c in rng.choice(CAP, size=8, replace=False))]),
         ("b. 2048 sets of 4 consecutive columns", [list(range(4 * j, 4 * j + 4)) for j in range(2048)]),
         ("c. 128 sets of 64 scattered members", [sorted(int(c) for c in rng.choice(CAP, size=64, replace=False)) for _ in range(128)]),
         ("d. one set of all 8192 columns", [list(range(CAP))])]


def alternative(ctx, g, sets):
    """export_filters -> OR on the host -> insert_filters into a fresh group: (the group, seconds export / OR / insert)"""
    alt = ka.Group(ctx, K, NH, L, max(len(sets), 128))
    ors = np.zeros((len(sets), max(1, nrows // 8)), dtype=np.uint8)
    t_export = t_or = 0.0
    flat = [c for s in sets for c in s]
    ends = np.cumsum([len(s) for s in sets])
    for at in range(0, len(flat), 256):           # (blocks of 256 members, whatever sets they belong to: a host image of 256 x 2^L / 8 bytes at a time)
        t0 = time.perf_counter()
        f = g.export_filters(flat[at:at + 256])
        t1 = time.perf_counter()
        j = int(np.searchsorted(ends, at, side="right"))
        while j < len(sets) and ends[j] - len(sets[j]) < at + len(f):
            lo, hi = max(int(ends[j]) - len(sets[j]), at) - at, min(int(ends[j]), at + len(f)) - at
            np.bitwise_or(ors[j], np.bitwise_or.reduce(f[lo:hi], axis=0), out=ors[j])
            j += 1
        t_export, t_or = t_export + t1 - t0, t_or + time.perf_counter() - t1
    t0 = time.perf_counter()
    assert alt.insert_filters(ors) == 0
    return alt, t_export, t_or, time.perf_counter() - t0


with ka.Context(0) as ctx:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
    warm, warm2 = ka.Group(ctx, K, NH, 10, CAP), ka.Group(ctx, K, NH, 10, CAP)      # (a kernel's first launch loads its code object: not timed)
    warm.add_random_columns(CAP, 1, 64)
    warm2.union_columns([[0, 1]], warm)
    warm2.insert_filters(warm.export_filters([0]))
    warm.close()
    warm2.close()
    g = ka.Group(ctx, K, NH, L, CAP)
    try:
        assert g.add_random_columns(CAP, 7, 64) == 0
        g.finalize()
        print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
        for what, sets in CASES:
            stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
            lines = np.unique(np.concatenate([np.asarray(s) // 512 for s in sets])).size
            bytes_in = nrows * 64 * lines
            ms, walls = [], []
            for _ in range(args.repeat):
                dst = ka.Group(ctx, K, NH, L, max(len(sets), 128))
                try:
                    t0 = time.perf_counter()
                    first, st = dst.union_columns(sets, g, timing=True)
                    walls.append(time.perf_counter() - t0)
                    ms.append(st["kernel_ms"])
                finally:
                    dst.close()
            moved = bytes_in + st["bytes_written"]
            loads_per_lane = st["entries"] / st["units"]
            print("union %-38s sets=%4d members=%6d entries=%5d units [%d, %d)  kernel ms %s  in %.3f GB (%d lines of a row) + out %.3f GB -> %.0f GB/s (best of %d);  "
                  "%.0f dword loads per lane -> %.1f G loads/s;  kwage_stream_read_gbps %.0f GB/s;  in+out rate / stream rate %.3f"
                  % (what, st["sets"], st["members"], st["entries"], st["first_unit"], st["first_unit"] + st["units"], " ".join("%.3f" % x for x in ms),
                     bytes_in / 1e9, lines, st["bytes_written"] / 1e9, moved / min(ms) / 1e6, args.repeat,
                     loads_per_lane, st["entries"] * nrows / min(ms) / 1e6, stream, moved / min(ms) / 1e6 / stream))
            if not args.no_alternative:
                t0 = time.perf_counter()
                alt, t_export, t_or, t_insert = alternative(ctx, g, sets)
                t_alt = time.perf_counter() - t0
                dst = ka.Group(ctx, K, NH, L, max(len(sets), 128))
                dst.union_columns(sets, g)
                rows = np.random.default_rng(1).choice(nrows, size=256, replace=False)
                assert np.array_equal(dst.read_rows(rows), alt.read_rows(rows))
                dst.close()
                alt.close()
                print("        wall: export %.2f s + OR %.2f s + insert %.2f s, in all %.2f s; the union call %.4f s (%.0f x)"
                      % (t_export, t_or, t_insert, t_alt, min(walls), t_alt / min(walls)))
            else:
                print("        wall: the union call %.4f s" % min(walls))
    finally:
        g.close()
