#!/usr/bin/env python3
"""kwage_topk_merge_device timings: R top-k lists of Q queries x k records each (what R ranks send rank 0 in
kwage_top_node), merged on the device, against a numpy merge of the same lists on the host.

The lists are made on the device: source r gives query q the columns j*R + r (j < k), so that no (query, column) pair
repeats, with scores drawn from [0, 64) -- many ties, broken by the column.  They lie source after source, as an exchange
leaves them.  Device times are host clocks around the synchronous call (kernels, the two 8-byte copies back and the
stream synchronisation; the context's streams are its own, so events on another stream cannot bracket it): the median
of --reps calls after --warmup.  The per-kernel split comes from a profiler run of this script (rocprofv3
--kernel-trace --stats).  The host merge is numpy's lexsort by (query, score descending, column) and a cut at k per
query, timed (the best of 3 runs) on at most --host-queries queries and scaled to Q linearly (reported as host_ms_scaled, with the
queries it ran on).  The device output is checked against the host merge on those queries.  One JSON line per shape.
   python tools/bench_topk_merge.py [--queries 100000] [--sources 2,8] [--k 10,1024] [--reps 5] [--warmup 2]
KWAGE_TOPK_MERGE_WAVE=0 / 1 forces the select kernel's workgroup / one-wave form (default: chosen by bucket size)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import kwage_amd as ka
from kwage_amd.native import check, lib


def make_lists(n_queries, k, sources, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = n_queries * k
    rows = torch.empty((sources * n, 3), dtype=torch.int32, device="cuda")
    q = torch.arange(n_queries, dtype=torch.int32, device="cuda").repeat_interleave(k)
    j = torch.arange(k, dtype=torch.int32, device="cuda").repeat(n_queries)
    for r in range(sources):
        blk = rows[r * n:(r + 1) * n]
        blk[:, 0] = q
        blk[:, 1] = j * sources + r
        blk[:, 2] = torch.randint(0, 64, (n,), dtype=torch.int32, device="cuda", generator=g)
    del q, j
    torch.cuda.synchronize()
    return rows


def host_merge(rows, k):
    q, c, m = rows[:, 0], rows[:, 1], rows[:, 2]
    idx = np.lexsort((c, -m.astype(np.int64), q))
    qs = q[idx]
    keep = idx[(np.arange(len(idx)) - np.searchsorted(qs, qs, side="left")) < k]
    out = rows[keep]
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--sources", default="2,8")
    ap.add_argument("--k", default="10,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-queries", type=int, default=2000)
    a = ap.parse_args()
    ctx = ka.Context(0)
    L = lib()
    try:
        for k in (int(x) for x in a.k.split(",")):
            for R in (int(x) for x in a.sources.split(",")):
                rows = make_lists(a.queries, k, R, 1000 * k + R)
                n = rows.shape[0]
                out = torch.empty((a.queries * k, 3), dtype=torch.int32, device="cuda")
                cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                call = lambda: check(L.kwage_topk_merge_device(ctx._h, rows.data_ptr(), n, a.queries, k, None, 0,
                                                               out.data_ptr(), out.shape[0], cnt.data_ptr()))
                for _ in range(a.warmup):
                    call()
                walls = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    walls.append((time.perf_counter() - t0) * 1e3)
                n_out = int(cnt.item())
                # the host merge on the first host_queries queries of every source, and the device output checked there
                hq = min(a.host_queries, a.queries)
                per = a.queries * k
                sub = torch.cat([rows[r * per:r * per + hq * k] for r in range(R)]).cpu().numpy()
                host_runs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    exp = host_merge(sub, k)
                    host_runs.append((time.perf_counter() - t0) * 1e3)
                host_ms = min(host_runs)
                got = out[:hq * k].cpu().numpy()
                assert n_out == a.queries * k and np.array_equal(got, exp), (k, R)
                dev_ms = statistics.median(walls)
                host_scaled = host_ms * a.queries / hq
                print(json.dumps({"run": "topk_merge", "sources": R, "queries": a.queries, "k": k, "records_in": n,
                                  "records_out": n_out, "device_ms": round(dev_ms, 3), "device_ms_min": round(min(walls), 3),
                                  "mrecords_per_s": round(n / dev_ms / 1e3, 1), "host_ms_scaled": round(host_scaled, 1),
                                  "host_queries": hq, "speedup": round(host_scaled / dev_ms, 1),
                                  "select_form": os.environ.get("KWAGE_TOPK_MERGE_WAVE", "auto")}), flush=True)
                del rows, out, cnt
                torch.cuda.empty_cache()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
