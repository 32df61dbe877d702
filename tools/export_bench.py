#!/usr/bin/env python3
"""Export (kwage_group_export_filters_device) measured beside its yardsticks, on one box in one process, on
compact_bench.py's group (2^L rows, 8192 random columns, rows 1 KiB apart).  The group is only read, so one group serves
every case:

  a. 1 column
  b. 32 columns
  c. 1024 consecutive columns
  d. 1024 columns taken every 8th

Per case: the export kernel's HIP-event time (device form: one launch over all rows) with the bytes written per second
(n filters of 2^L / 8 bytes), and, in the same process,

  1. kwage_stream_read_gbps of the same matrix: what the box streams from it;
  2. the insert kernel's time (insert_kernel_ms) for the same n filters -- the ones just exported -- into a fresh group:
     the mirror operation;
  3. the extract kernel's time (kwage_save_stats.extract_kernel_ms) when kwage_group_save_db saves the same column list:
     the same reads without the transpose.

    python tools/export_bench.py [--log2 23] [--tmp DIR] [--no-save]"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (a one-shot program: no second candidate block for the matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka
from kwage_amd.native import check, lib

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=23)
ap.add_argument("--tmp", default=None)
ap.add_argument("--no-save", action="store_true", help="leave out the saves (yardstick 3): no file is written")
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
nrows = 1 << L
fb = max(1, nrows // 8)
tmp = tempfile.mkdtemp(prefix="export_bench_", dir=args.tmp)

CASES = [("a. 1 column", [4097]),
         ("b. 32 columns", list(range(4100, 4132))),
         ("c. 1024 consecutive columns", list(range(2048, 3072))),
         ("d. 1024 columns, every 8th", list(range(3, CAP, 8)))]


def insert_ms(ctx, dev, n, log2=L):
    """insert_kernel_ms of the n filters in `dev` into a fresh group"""
    g = ka.Group(ctx, K, NH, log2, max(n, 128))
    try:
        first, ms = C.c_uint64(), C.c_float(0)
        check(lib().kwage_group_insert_filters_device(g._h, dev.data_ptr(), dev.stride(0), n, ka.SEARCH_TIMING, C.byref(first), C.byref(ms)))
        return ms.value
    finally:
        g.close()


try:
    import torch
    with ka.Context(0) as ctx:
        print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
        device = torch.device("cuda", ctx.device)
        warm = ka.Group(ctx, K, NH, 10, CAP)          # (a kernel's first launch loads its code object: not timed)
        warm.add_random_columns(CAP, 1, 64)
        w = torch.empty((40, 128), dtype=torch.uint8, device=device)
        warm.export_filters(list(range(40)), out=w)
        insert_ms(ctx, w, 40, 10)
        warm.close()
        g = ka.Group(ctx, K, NH, L, CAP)
        try:
            assert g.add_random_columns(CAP, 7, 64) == 0
            g.finalize()
            print("group: 2^%d rows, %d random columns at density 1/4 (row stride %d bytes, %.2f GB resident)" % (L, CAP, g.row_stride, g.device_bytes / 1e9))
            stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
            for what, cols in CASES:
                n = len(cols)
                dev = torch.empty((n, fb), dtype=torch.uint8, device=device)
                g.export_filters(cols, out=dev, timing=True)                  # (once untimed: the output's pages are touched)
                times = sorted(g.export_filters(cols, out=dev, timing=True)[1] for _ in range(3))
                ms = times[1]
                line = "export %-30s n=%4d  kernel ms %.3f (of 3: %.3f .. %.3f)  out %.3f GB -> %.1f GB/s written" % (
                    what, n, ms, times[0], times[2], n * fb / 1e9, n * fb / ms / 1e6)
                ins = insert_ms(ctx, dev, n)
                line += ";  insert of the same %d filters into a fresh group: kernel ms %.3f (export / insert = %.2f)" % (n, ins, ms / ins)
                if not args.no_save:
                    out = os.path.join(tmp, "saved.db")
                    st = g.save_db(out, cols, [{"run_accession": "SRR%d" % (c + 1)} for c in cols])
                    os.remove(out)
                    line += ";  extract kernel (save of the same list) %.3f ms (export / extract = %.2f)" % (st["extract_kernel_ms"], ms / st["extract_kernel_ms"])
                print(line + ";  kwage_stream_read_gbps %.0f GB/s" % stream)
                del dev
        finally:
            g.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
