#!/usr/bin/env python3
"""Live insert (kwage_group_insert_filters*) measured beside its yardsticks, on one box in one process.

  1. the insert kernel's HIP-event time for n filters at tail offsets s (device form: filters resident, one launch), with
     bytes in + out per second -- in: n filters of 2^L / 8 bytes; out: 2^L rows x the 32-bit words the call owns;
  2. kwage_build_db's transpose_kernel_ms (kwage_build_stats) for the same numbers of filters: the same bits, the same
     transpose, packed instead of strided output -- in + out = 2 x n x 2^L / 8 bytes;
  3. for n = 1 the sector-traffic floor of DESIGN.md section 15: every row takes one 32-byte sector, at the rate the
     box streams its own matrix (kwage_stream_read_gbps);
  4. wall time until m new samples are searchable in a resident group: kwage_group_insert_bloom_files against the only
     route without it -- kwage_build_db of the new files, destroy, reload of the group (the resident `.db` and the new one).

    python tools/insert_bench.py [--log2 23] [--capacity 16384] [--ns 1,64,1024,8192] [--offsets 0,5] [--build 1024,8192]
                                 [--searchable 1,1024] [--resident 1024] [--tmp DIR]"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np

# (a one-shot program: no second candidate block for the 17 GB matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka
from kwage_amd import native
import kwage_oracle as oracle

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=23)
ap.add_argument("--capacity", type=int, default=16384)
ap.add_argument("--ns", default="1,64,1024,8192")
ap.add_argument("--offsets", default="0,5")
ap.add_argument("--build", default="1024,8192")
ap.add_argument("--searchable", default="1,1024")
ap.add_argument("--resident", type=int, default=1024)
ap.add_argument("--tmp", default=None)
args = ap.parse_args()
ints = lambda s: [int(x) for x in s.split(",") if x]
L, K, NH = args.log2, 31, 1
fbytes = (1 << L) // 8
lib = native.lib()


def timed_insert_device(g, t, n):
    first, ms = C.c_uint64(), C.c_float()
    native.check(lib.kwage_group_insert_filters_device(g._h, t.data_ptr(), t.stride(0), n, ka.SEARCH_TIMING, C.byref(first), C.byref(ms)))
    g._real.append((first.value, n))
    return first.value, ms.value


with ka.Context(0) as ctx:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx.fingerprint().items()))
    print("group: 2^%d rows, capacity %d columns (row stride %d bytes); filters of %d bytes" % (L, args.capacity, (args.capacity + 7) // 8, fbytes))
    import torch
    dev = torch.device("cuda", ctx.device)
    ns = ints(args.ns)
    stream_gbps = None
    if ns:
        pool = torch.randint(0, 256, (max(ns), fbytes), dtype=torch.uint8, device=dev)
        for s in ints(args.offsets):
            g = ka.Group(ctx, K, NH, L, args.capacity)
            try:
                if stream_gbps is None:
                    stream_gbps = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
                    print("the box streams its matrix at %.0f GB/s (kwage_stream_read_gbps)" % stream_gbps)
                if s:
                    timed_insert_device(g, pool, s)
                for n in sorted(ns, reverse=True):          # (multiples of 32 first: the offset stays s; single filters last)
                    reps = 1 if n > 2048 else 3
                    runs = []
                    for _ in range(reps):
                        if g.column_span + n + 32 > args.capacity:
                            break
                        first, ms = timed_insert_device(g, pool, n)
                        words = (first + n - 1) // 32 - first // 32 + 1
                        runs.append((first, ms, (n * fbytes + (1 << L) * words * 4) / ms / 1e6))
                    for first, ms, gbps in runs:
                        line = "insert kernel: n = %5d at column %6d (s = %2d): %9.1f us, %7.1f GB/s in + out" % (n, first, first % 32, ms * 1e3, gbps)
                        if n == 1:
                            floor_us = (1 << L) * 32 / stream_gbps / 1e3
                            line += "; floor (one 32-byte sector per row at the streaming rate) %.1f us: %.2fx the floor" % (floor_us, ms * 1e3 / floor_us)
                        print(line)
            finally:
                g.close()
        del pool
        torch.cuda.empty_cache()

    builds, searchable = ints(args.build), ints(args.searchable)
    nfiles = max(builds + [args.resident + max(searchable + [0])] + [0])
    if nfiles:
        tmp = tempfile.mkdtemp(prefix="kwage_insert_", dir=args.tmp)
        try:
            free = shutil.disk_usage(tmp).free
            need = lambda n: 2 * n * fbytes + (1 << 30)
            rng = np.random.default_rng(3)
            payloads = [rng.integers(0, 256, size=fbytes, dtype=np.uint8) & rng.integers(0, 256, size=fbytes, dtype=np.uint8) for _ in range(8)]
            paths = []

            def files(n):
                while len(paths) < n:
                    j = len(paths)
                    p = os.path.join(tmp, "f%05d.bloom" % j)
                    oracle.write_bloom(p, K, L, NH, oracle.FilterInfo(run_accession=oracle.str_to_accession("SRR%d" % (j + 1))), payloads[j % len(payloads)])
                    paths.append(p)
                return paths[:n]

            def build(ps, out):
                arr = (C.c_char_p * len(ps))(*[p.encode() for p in ps])
                prm, st = native.Params(K, NH, L, 0), native.BuildStats()
                t0 = time.perf_counter()
                native.check(lib.kwage_build_db(ctx._h, out.encode(), C.byref(prm), arr, len(ps), C.byref(st)))
                return time.perf_counter() - t0, st.transpose_kernel_ms

            def builder_line(n):
                if need(n) > free:
                    print("builder: n = %d skipped: %d GiB of scratch files needed, %d GiB free" % (n, need(n) >> 30, free >> 30))
                    return
                out = os.path.join(tmp, "build.db")
                best = min(build(files(n), out)[1] for _ in range(1 if n > 2048 else 2))
                os.remove(out)
                print("builder kernel (transpose_kernel_ms): n = %5d: %9.1f us, %7.1f GB/s in + out" % (n, best * 1e3, 2 * n * fbytes / best / 1e6))

            for n in [n for n in builds if n <= 2048]:
                builder_line(n)

            if searchable and need(args.resident + max(searchable)) <= free:
                resident = os.path.join(tmp, "resident.db")
                build(files(args.resident), resident)

                def load(dbs):
                    g = ka.Group(ctx, K, NH, L, args.capacity)
                    g.add_db_files(dbs)
                    g.finalize()
                    return g
                query = ka.Batch(ctx, ["ACGT" * 20])
                for m in searchable:
                    new = files(args.resident + m)[args.resident:]
                    g = load([resident])
                    t0 = time.perf_counter()
                    g.insert_bloom_files(new)
                    t_insert = time.perf_counter() - t0
                    g.search(query, 1.0)
                    # the route without the insert: a `.db` of the new files, destroy, reload at the same size
                    t0 = time.perf_counter()
                    newdb = os.path.join(tmp, "new.db")
                    build(new, newdb)
                    t_build = time.perf_counter() - t0
                    g.close()
                    g = load([resident, newdb])
                    t_reload = time.perf_counter() - t0
                    g.search(query, 1.0)
                    g.close()
                    os.remove(newdb)
                    print("searchable: %4d new sample(s) beside %d resident columns: live insert %.1f us wall; build_db + destroy + reload %.1f us wall "
                          "(build_db %.1f us of it): %.0fx" % (m, args.resident, t_insert * 1e6, t_reload * 1e6, t_build * 1e6, t_reload / t_insert))
                query.close()
            elif searchable:
                print("searchable: skipped: not enough scratch space")
            for n in [n for n in builds if n > 2048]:          # (the many files of the large builds last)
                builder_line(n)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
