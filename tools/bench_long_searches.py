#!/usr/bin/env python3
"""The segmented path of the four counted searches on few long queries (4 x 1 Mb vs 100k samples: bench_long_query.py's
second workload, at t = 0.9): kwage_search (count_kernel<SEG> + count_combine_kernel), search_topk, search_scores_device
and search_presence_device (the same segment counts, then their own combine kernels), alternating repetition by
repetition in one process; kernel times are HIP-event times of the search stage, the median of 7 after 2 warm-ups, the
spread (max - min) / median.  Checksums of what the searches left come first: equal between two libraries on the same
seeded workload.  One JSON line per record, each with the device's fingerprint.
   python tools/bench_long_searches.py [TREE [LABEL]]     TREE: the tree whose kwage_amd package and library are used
                                                          (an A/B against another build: a copy of the tree with its
                                                          library); LABEL goes into every record"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
reps, warmup = 7, 2
import numpy as np

import kwage_amd as ka
from kwage_amd import synth
from kwage_amd.engine import presence_row_bytes

import torch

w = synth.Workload("long4", 100_000, 20, 31, 1, 4, 1_000_000, 0.9, num_genomes=4, genome_len=1_000_000, hit_fraction=1.0)
with ka.Context(0) as ctx:
    fp = ctx.fingerprint()

    def emit(**rec):
        rec["library"] = label
        rec["fingerprint"] = fp
        print(json.dumps(rec), flush=True)
    t0 = time.perf_counter()
    s = synth.build(ctx, w)
    g, b = s.group, s.batch
    n, span = b.n, g.column_span
    emit(setup="4 x 1 Mb vs 100k samples, 2^20-bit filters, 1 hash, t=0.9", build_s=round(time.perf_counter() - t0, 1), queries=int(n), span=int(span))
    T = ka.SEARCH_TIMING
    dev = "cuda:%d" % ctx.device
    scores = torch.empty((n, span), dtype=torch.int32, device=dev)
    bits = torch.empty((n, presence_row_bytes(g)), dtype=torch.uint8, device=dev)
    ctx.set_tuning("count_walk", 0)      # the segmented form, not the persistent count walk

    runs = [("kwage_search t=0.9", lambda: g.search(b, 0.9, T), lambda r: (r.search_kernel_ms, r.search_kernel)),
            ("search_topk k=10 t=0.9", lambda: ka.search_topk(g, b, 10, 0.9, T), lambda r: (r.search_kernel_ms, r.search_kernel)),
            ("search_scores_device", lambda: ka.search_scores_device(g, b, scores, flags=T), lambda r: (r.kernel_ms, r.kernel)),
            ("search_presence_device t=0.9", lambda: ka.search_presence_device(g, b, 0.9, bits, flags=T), lambda r: (r.kernel_ms, r.kernel))]
    ms = {name: [] for name, _, _ in runs}
    wall = {name: [] for name, _, _ in runs}
    kern = {}
    for rep in range(warmup + reps):
        for name, fn, get in runs:
            t1 = time.perf_counter()
            r = fn()
            dt = (time.perf_counter() - t1)*1e3
            k_ms, kern[name] = get(r)
            if rep >= warmup:
                ms[name].append(float(k_ms))
                wall[name].append(dt)
    # a checksum of what the searches left: equal across libraries on the same seeded workload
    r = g.search(b, 0.9, T)
    sums = {"hits": int(len(r.hits)), "hit_sum": int(r.hits["num_match"].astype(np.uint64).sum() + r.hits["column"].astype(np.uint64).sum()),
            "scores_sum": int(scores.to(torch.int64).sum().item()),
            "bits_bytes_sum": int(bits.to(torch.int64).sum().item())}
    emit(check="checksums of the results", **sums)
    for name, _, _ in runs:
        v = ms[name]
        med = statistics.median(v)
        emit(run=name, kernel=kern[name], kernel_ms=round(med, 4), spread=round((max(v) - min(v))/med, 4), wall_ms=round(statistics.median(wall[name]), 3),
             reps=reps, all_ms=[round(x, 4) for x in v])
    s.batch.close(); s.group.close()
