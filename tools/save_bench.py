#!/usr/bin/env python3
"""Save (kwage_group_save_db) measured beside its yardsticks, on one box in one process, on a 2^L-row group:

  1. the extract kernel's HIP-event time (kwage_save_stats.extract_kernel_ms, summed over the staged chunks) for
       a. 2048 contiguous columns            (one run; out_slice 256: the 16-byte path),
       b. 8192 contiguous columns            (one run; out_slice 1024),
       c. 2048 columns with every 64th column of the range retired   (runs of 63 columns),
     the 2048-column lists with the default 64 MiB staging chunks and with 1 GiB chunks (fewer, longer launches),
     with bytes in + out per second -- in: ceil(n / 8) wanted bytes per row, out: the same packed;
  2. kwage_stream_read_gbps of the same group: what the box streams from its own matrix;
  3. kwage_build_db's transpose_kernel_ms (kwage_build_stats) for 2048 filters of the same length: the builder's kernel
     writes the same packed block from filter-major input -- in + out = 2 x 2048 x 2^L / 8 bytes.

    python tools/save_bench.py [--log2 23] [--repeat 2] [--tmp DIR] [--no-build]"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np

# (a one-shot program: no second candidate block for the matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka
from kwage_amd import native
import kwage_oracle as oracle

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=23)
ap.add_argument("--repeat", type=int, default=2)
ap.add_argument("--tmp", default=None)
ap.add_argument("--no-build", action="store_true")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
nrows = 1 << L
lib = native.lib()
tmp = tempfile.mkdtemp(prefix="save_bench_", dir=args.tmp)


def measure(g, what, columns, staging=0, repeat=None):
    n = len(columns)
    out = os.path.join(tmp, "saved.db")
    sources = [{"run_accession": "SRR%d" % (c + 1)} for c in columns]
    ms, wall, st = [], [], None
    for _ in range((repeat or args.repeat) + 1):     # the first one warms up (pinned blocks, page cache)
        t0 = time.perf_counter()
        st = g.save_db(out, columns, sources, staging)
        wall.append(time.perf_counter() - t0)
        ms.append(st["extract_kernel_ms"])
        os.remove(out)
    ms, wall = ms[1:], wall[1:]
    moved = 2 * nrows * ((n + 7) // 8)
    med = statistics.median(ms)
    print("save %-40s n=%5d runs=%4d chunks=%3d  extract kernel ms %s  median %.3f  in+out %.3f GB -> %.0f GB/s  (file %.2f GB, wall median %.2f s)"
          % (what, n, st["runs"], st["chunks"], " ".join("%.3f" % x for x in ms), med, moved / 1e9, moved / med / 1e6, st["db_bytes"] / 1e9, statistics.median(wall)))


try:
    with ka.Context(0) as ctx:
        print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
        g = ka.Group(ctx, K, NH, L, CAP)
        try:
            print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
            assert g.add_random_columns(CAP, 7, 64) == 0
            print("kwage_stream_read_gbps of the group: %.0f GB/s" % g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3))
            measure(g, "2048 contiguous", list(range(2048)))
            measure(g, "2048 contiguous, 1 GiB chunks", list(range(2048)), 1 << 30)
            measure(g, "8192 contiguous", list(range(CAP)), repeat=1)           # (an 8.6 GB file per save)
            gone = [c for c in range(4096, 4096 + 2112) if c % 64 == 63]
            g.retire_columns(gone)
            holes = [c for c in range(4096, 4096 + 2112) if c % 64 != 63][:2048]
            measure(g, "2048, every 64th retired", holes)
            measure(g, "2048, every 64th retired, 1 GiB chunks", holes, 1 << 30)
        finally:
            g.close()
        if not args.no_build:
            rng = np.random.default_rng(1)
            n = 2048
            paths = []
            bits = rng.integers(0, 256, size=nrows // 8, dtype=np.uint8)
            for j in range(n):
                p = os.path.join(tmp, "f%05d.bloom" % j)
                bits[: 1 << 10] = rng.integers(0, 256, size=1 << 10, dtype=np.uint8)        # (files that differ; the kernel's time does not depend on the bits)
                oracle.write_bloom(p, K, L, NH, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (j + 1))), bits)
                paths.append(p)
            arr = (C.c_char_p * n)(*[p.encode() for p in paths])
            prm = native.Params(K, NH, L, 0)
            ms = []
            for _ in range(args.repeat + 1):
                st = native.BuildStats()
                db = os.path.join(tmp, "built.db")
                native.check(lib.kwage_build_db(ctx._h, db.encode(), C.byref(prm), arr, n, C.byref(st)))
                ms.append(st.transpose_kernel_ms)
                os.remove(db)
            ms = ms[1:]
            moved = 2 * n * (nrows // 8)
            med = statistics.median(ms)
            print("kwage_build_db %d filters of 2^%d bits: transpose kernel ms %s  median %.3f  in+out %.3f GB -> %.0f GB/s"
                  % (n, L, " ".join("%.3f" % x for x in ms), med, moved / 1e9, moved / med / 1e6))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
