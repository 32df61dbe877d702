#!/usr/bin/env python3
"""Presence search timings at the C2 shape (100 k samples x 2^23-bit filters, 1 k x 1 kb queries, 1 hash;
kwage_amd/synth.py), in one process on one box, the seven runs alternating repetition by repetition:

  (a) kwage_search at t = 0.8 without early exit, the tiled count_kernel forced (knob count_walk = 0)
  (b) search_scores_device: the dense matrix of the same loop
  (c) search_presence_device at t = 0.8 without KWAGE_SEARCH_EARLY_EXIT
  (d) the same with the flag
  (e) kwage_search at t = 1 on the tiled and_kernel without early exit (knob walk = 0)
  (f) search_presence_device at t = 1 without the flag
  (g) the same with the flag

Kernel times are HIP-event times of the search stage, the median of --reps repetitions after --warmup; the spread is
(max - min) / median over the repetitions.  Presence runs the loop of (b) and of (a), writes 1/32 of (b)'s bytes and
expands nothing, so the expectations tested are

    (c) <= (b) * (1 + margin)        (f) <= (e) * (1 + margin)

with margin = the largest spread any of the seven runs recorded in this process.  (d)/(c) and (g)/(f) are reported as
ratios without a target: what the per-tile exit gains depends on how many tiles hold a passing column.

Before timing, a sample of rows of (c), (d), (f) and (g) is checked against the hit lists of (a) and (e): the set columns
are the listed columns, exactly.  One JSON line per record, each with the device's fingerprint.
   python tools/bench_presence.py [--log2 23] [--samples 100000] [--reps 7] [--warmup 2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=23)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=24)
    a = ap.parse_args()
    assert a.reps >= 5
    import torch
    w = dataclasses.replace(synth.WORKLOADS["c2"], num_samples=a.samples, log_2_filter_len=a.log2, num_queries=a.queries,
                            threshold=0.8)
    with ka.Context(0) as ctx:
        fp = ctx.fingerprint()

        def emit(**rec):
            rec["fingerprint"] = fp
            print(json.dumps(rec), flush=True)
            return rec
        t0 = time.perf_counter()
        s = synth.build(ctx, w)
        g, b = s.group, s.batch
        n, span = b.n, g.column_span
        wbytes = (g.row_bytes + 15) // 16 * 16
        emit(setup=w.name, samples=a.samples, log2=a.log2, queries=a.queries, span=int(span), row_bytes=int(wbytes),
             build_s=round(time.perf_counter() - t0, 1))
        T, EE = ka.SEARCH_TIMING, ka.SEARCH_EARLY_EXIT
        dev = "cuda:%d" % ctx.device
        scores = torch.empty((n, span), dtype=torch.int32, device=dev)
        bits = torch.empty((n, wbytes), dtype=torch.uint8, device=dev)

        def run_a():
            with ctx.tuning(count_walk=0):
                return g.search(b, 0.8, T)

        def run_b():
            return ka.search_scores_device(g, b, scores, flags=T)

        def run_e():
            with ctx.tuning(walk=0):
                return g.search(b, 1.0, T)

        def presence(t, flags):
            return lambda: ka.search_presence_device(g, b, t, bits, flags=T | flags)

        # ---- exactness first: sampled rows of the four presence runs against the hit lists of (a) and (e) ---------------------
        rows = sorted(set(np.linspace(0, n - 1, a.check_rows).astype(int).tolist()))
        for t, ref, kernel in ((0.8, run_a(), "count_kernel<"), (1.0, run_e(), "and_kernel<")):
            assert ref.search_kernel.startswith(kernel), ref.search_kernel
            hq = ref.hits["query"]
            for flags in (0, EE):
                bits.fill_(0xFF)
                res = presence(t, flags)()
                for q in rows:
                    row = np.unpackbits(bits[q].cpu().numpy(), bitorder="little")
                    lo, hi = np.searchsorted(hq, q, "left"), np.searchsorted(hq, q, "right")
                    assert np.array_equal(np.flatnonzero(row), ref.hits[lo:hi]["column"]), (t, flags, q)
                emit(check="rows of search_presence_device against kwage_search", t=t, early_exit=bool(flags), rows=len(rows),
                     kernel=res.kernel, reference_kernel=ref.search_kernel, equal=True)

        # ---- timing: the seven runs alternating ---------------------------------------------------------------------------------
        runs = [("a", run_a, "kwage_search t=0.8, tiled count_kernel, no early exit"),
                ("b", run_b, "search_scores_device"),
                ("c", presence(0.8, 0), "search_presence_device t=0.8"),
                ("d", presence(0.8, EE), "search_presence_device t=0.8, early exit"),
                ("e", run_e, "kwage_search t=1, tiled and_kernel, no early exit"),
                ("f", presence(1.0, 0), "search_presence_device t=1"),
                ("g", presence(1.0, EE), "search_presence_device t=1, early exit")]
        ms = {name: [] for name, _, _ in runs}
        wall = {name: [] for name, _, _ in runs}
        kernels = {}
        for rep in range(a.warmup + a.reps):
            for name, fn, _ in runs:
                t1 = time.perf_counter()
                r = fn()
                dt = (time.perf_counter() - t1) * 1e3
                kernels[name] = r.search_kernel if hasattr(r, "search_kernel") else r.kernel
                if rep >= a.warmup:
                    ms[name].append(float(r.search_kernel_ms if hasattr(r, "search_kernel_ms") else r.kernel_ms))
                    wall[name].append(dt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()}
        for name, _, label in runs:
            emit(run="(%s) %s" % (name, label), kernel=kernels[name], kernel_ms=round(med[name], 4), spread=round(spread[name], 4),
                 wall_ms=round(statistics.median(wall[name]), 3), reps=a.reps, all_ms=[round(x, 4) for x in ms[name]])
        margin = max(spread.values())
        for mine, ref in (("c", "b"), ("f", "e")):
            ratio = med[mine] / med[ref]
            emit(expectation="(%s) <= (%s) within the largest spread of the run" % (mine, ref), ratio=round(ratio, 4), margin=round(margin, 4),
                 met=bool(ratio <= 1 + margin), missed_by=round(max(0.0, ratio - 1 - margin), 4),
                 bytes_written=int(n) * int(wbytes), bytes_written_by_scores=int(n) * int(span) * 4)
        emit(ratio="(c)/(a)", value=round(med["c"] / med["a"], 4))
        emit(ratio="(d)/(c): what the per-tile exit gains at t=0.8 (no target)", value=round(med["d"] / med["c"], 4))
        emit(ratio="(g)/(f): what the per-tile exit gains at t=1 (no target)", value=round(med["g"] / med["f"], 4))


if __name__ == "__main__":
    main()
