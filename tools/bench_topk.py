#!/usr/bin/env python3
"""Top-k search timings at the C2 shape (100 k samples x 2^23-bit filters, 1 k x 1 kb queries, 1 hash; kwage_amd/synth.py):
kwage_search_topk for k in {1, 10, 100, 1024} and t in {0, 0.8}, against kwage_search at t = 0.8 (the library's own
choice, and the tiled count_kernel forced) and the low-threshold route top-k replaces (a threshold whose floor is 0:
every column is a hit, then the host keeps the k best per query).

Kernel times are HIP-event times of the search stage (kwage_result.search_kernel_ms: for top-k the tile / segment
kernels and the per-query merge), the median of --reps runs after --warmup; GB/s is the algorithmic bytes (every
addressed row's bytes of the real columns) over that time, and frac is that over the 8 TB/s HBM peak, as bench.py
reports it.  Wall times are host clocks around the whole call (k-mer stage, copies and result assembly included).
One JSON line per measurement.
   python tools/bench_topk.py [--log2 23] [--samples 100000] [--reps 5] [--warmup 2] [--no-low]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import kwage_amd as ka
from kwage_amd import synth

HBM_PEAK_GBPS = 8000.0


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ks, ws, r = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ws.append((time.perf_counter() - t0) * 1e3)
        ks.append(r.search_kernel_ms)
    return statistics.median(ks), statistics.median(ws), r


def line(name, k_ms, wall_ms, r, **extra):
    gbps = r.algorithmic_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None
    rec = {"run": name, "kernel": r.search_kernel, "kernel_ms": round(k_ms, 4), "wall_ms": round(wall_ms, 3),
           "algorithmic_bytes": int(r.algorithmic_bytes), "gbps": round(gbps, 1) if gbps else None,
           "frac": round(gbps / HBM_PEAK_GBPS, 4) if gbps else None, "hits": int(r.hits.size)}
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=23)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-low", action="store_true", help="skip the low-threshold route (a 100 M-record hit list at C2)")
    a = ap.parse_args()
    w = dataclasses.replace(synth.WORKLOADS["c2"], num_samples=a.samples, log_2_filter_len=a.log2, num_queries=a.queries,
                            threshold=0.8)
    with ka.Context(0) as ctx:
        t0 = time.perf_counter()
        s = synth.build(ctx, w)
        print(json.dumps({"setup": w.name, "samples": a.samples, "log2": a.log2, "queries": a.queries,
                          "build_s": round(time.perf_counter() - t0, 1), "device": ctx.fingerprint().get("name")}), flush=True)
        g, b = s.group, s.batch
        T = ka.SEARCH_TIMING
        base = line("kwage_search t=0.8", *measure(lambda: g.search(b, 0.8, T), a.reps, a.warmup))
        with ctx.tuning(count_walk=0):
            tiled = line("kwage_search t=0.8 count_kernel", *measure(lambda: g.search(b, 0.8, T), a.reps, a.warmup))
        for t in (0.0, 0.8):
            for k in (1, 10, 100, 1024):
                rec = line("search_topk k=%d t=%.1f" % (k, t), *measure(lambda: ka.search_topk(g, b, k, t, T), a.reps, a.warmup))
                if k == 10 and t == 0.8:
                    print(json.dumps({"ratio_topk10_to_count_kernel": round(rec["kernel_ms"] / tiled["kernel_ms"], 3),
                                      "ratio_topk10_to_search": round(rec["kernel_ms"] / base["kernel_ms"], 3)}), flush=True)
        if not a.no_low:
            # the route top-k replaces: every column a hit (floor 0), copied back, the k best kept per query on the host
            low_t = 1e-4
            for k in (10,):
                def low():
                    r = g.search(b, low_t, T)
                    h = r.hits
                    order = np.lexsort((h["column"], -h["num_match"].astype(np.int64), h["query"]))
                    hq = h["query"][order]
                    first = np.searchsorted(hq, hq, side="left")
                    keep = order[(np.arange(order.size) - first) < k]
                    r.kept = int(keep.size)
                    return r
                line("low-threshold route t=1e-4 + host top-%d" % k, *measure(low, max(1, a.reps // 2), 1),
                     hit_bytes=int(g.num_columns) * a.queries * 12)


if __name__ == "__main__":
    main()
