#!/usr/bin/env python3
"""Compaction (kwage_group_compact) measured beside its yardsticks, on one box in one process, on save_bench.py's group
(2^L rows, 8192 random columns, rows 1 KiB apart).  A compaction changes its group, so every case gets a fresh one:

  a. column 0 retired             one long run, every unit shifted by one bit
  b. every 64th column retired    every unit crossed by a run boundary: the walked path
  c. the last 1024 columns retired    nothing moves: only the units at and above m are written, as zeros

Per case: the kernel's HIP-event time (kwage_compact_stats.kernel_ms) with bytes in + out per second -- in: the bytes of a
row from the first unit rewritten to the last survivor, out: the units written -- and, in the same process,

  1. kwage_stream_read_gbps of the same matrix: what the box streams from it;
  2. the extract kernel's rate (kwage_save_stats.extract_kernel_ms) when kwage_group_save_db saves the same survivors
     before the compaction: the same bytes through the same arithmetic, into a second buffer;
  3. for case b, the wall time of save + destroy + load (the round trip through a `.db` file that was the only way to
     give retired columns' space back) against the wall time of the compaction call.

    python tools/compact_bench.py [--log2 23] [--tmp DIR] [--no-save]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (a one-shot program: no second candidate block for the matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=23)
ap.add_argument("--tmp", default=None)
ap.add_argument("--no-save", action="store_true", help="leave out the saves (yardsticks 2 and 3): no file is written")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
nrows = 1 << L
tmp = tempfile.mkdtemp(prefix="compact_bench_", dir=args.tmp)

CASES = [("a. column 0 retired", [0], False),
         ("b. every 64th column retired", list(range(63, CAP, 64)), True),
         ("c. the last 1024 columns retired", list(range(CAP - 1024, CAP)), False)]


def fresh(ctx, gone):
    g = ka.Group(ctx, K, NH, L, CAP)
    assert g.add_random_columns(CAP, 7, 64) == 0
    g.finalize()
    g.retire_columns(gone)
    return g


try:
    with ka.Context(0) as ctx:
        print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
        warm = ka.Group(ctx, K, NH, 10, CAP)          # (the kernel's first launch loads its code object: not timed)
        warm.add_random_columns(CAP, 1, 64)
        warm.retire_columns([0])
        warm.compact()
        warm.close()
        for what, gone, round_trip in CASES:
            g = fresh(ctx, gone)
            try:
                if what.startswith("a"):
                    print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
                stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
                gone_set = set(gone)
                keep = [c for c in range(CAP) if c not in gone_set]
                m = len(keep)
                line = ""
                t_save = t_close = t_load = 0.0
                if not args.no_save:
                    out = os.path.join(tmp, "saved.db")
                    t0 = time.perf_counter()
                    st = g.save_db(out, keep, [{"run_accession": "SRR%d" % (c + 1)} for c in keep])
                    t_save = time.perf_counter() - t0
                    moved = 2 * nrows * ((m + 7) // 8)
                    line = "  extract kernel (save of the same survivors) %.3f ms, in+out %.3f GB -> %.0f GB/s;" % (st["extract_kernel_ms"], moved / 1e9, moved / st["extract_kernel_ms"] / 1e6)
                    if round_trip:
                        t0 = time.perf_counter()
                        g.close()
                        t_close = time.perf_counter() - t0
                        t0 = time.perf_counter()
                        g2 = ka.Group(ctx, K, NH, L, CAP)
                        g2.add_db_file(out)
                        g2.finalize()
                        t_load = time.perf_counter() - t0
                        assert g2.num_columns == m
                        g2.close()
                        g = fresh(ctx, gone)
                    os.remove(out)
                t0 = time.perf_counter()
                new, cs = g.compact(timing=True)
                t_compact = time.perf_counter() - t0
                assert cs["columns"] == m and g.column_span == (m + 7) // 8 * 8
                bytes_in = nrows * max(0, (m + 7) // 8 - 16 * cs["first_unit"])
                bytes_out = nrows * 16 * cs["units"]
                print("compact %-34s m=%5d runs=%4d units [%d, %d)  kernel ms %.3f  in %.3f GB + out %.3f GB -> %.0f GB/s;%s  kwage_stream_read_gbps %.0f GB/s"
                      % (what, m, cs["runs"], cs["first_unit"], cs["first_unit"] + cs["units"], cs["kernel_ms"], bytes_in / 1e9, bytes_out / 1e9,
                         (bytes_in + bytes_out) / cs["kernel_ms"] / 1e6, line, stream))
                if round_trip and not args.no_save:
                    print("        wall: save %.2f s + destroy %.2f s + load %.2f s = %.2f s; the compaction call %.4f s (%.0f x)"
                          % (t_save, t_close, t_load, t_save + t_close + t_load, t_compact, (t_save + t_close + t_load) / t_compact))
                else:
                    print("        wall: the compaction call %.4f s" % t_compact)
            finally:
                g.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
