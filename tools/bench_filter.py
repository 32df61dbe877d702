#!/usr/bin/env python3
"""Filter search timings at the C2 shape (100 k samples x 2^23-bit filters, 1 hash; kwage_amd/synth.py), in one process on
one box, the runs alternating repetition by repetition (the protocol of profiles/r06_scores_bench.txt):

  (a) search_scores_device on a batch of --filters random sequences, each as long as one of (b)'s filters has set rows:
      the dense score search as it was before the filter search existed, in the same launch form over as many rows as a
      random genome allows (its distinct k-mers are its rows: one hash function)
  (b) search_filter_scores_device for --filters planted sample columns of the matrix itself
  (c) FilterSet.from_columns for the same columns: the extraction alone (wall time: the call is synchronous), against the
      time the box's streaming probe implies for one 64-byte sector per row and column

(a) and (b) are compared by algorithmic bytes per second: rows x row bytes / HIP-event time of the score stage.  The
expectation tested is (b) >= 0.95 (a).  Before timing, (b)'s cell at each filter's own column is checked against the
filter's bit count and the column's.  One JSON line per record, each with the device's fingerprint.
   python tools/bench_filter.py [--log2 23] [--samples 100000] [--filters 4] [--reps 7] [--warmup 2]"""
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
    ap.add_argument("--filters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.reps >= 5
    import torch
    w = dataclasses.replace(synth.WORKLOADS["c2"], num_samples=a.samples, log_2_filter_len=a.log2, num_queries=1)
    with ka.Context(0) as ctx:
        fp = ctx.fingerprint()

        def emit(**rec):
            rec["fingerprint"] = fp
            print(json.dumps(rec), flush=True)
            return rec
        t0 = time.perf_counter()
        s = synth.build(ctx, w)
        g = s.group
        span, row_bytes = g.column_span, g.row_bytes
        cols = [s.planted[i][0] for i in range(a.filters)]
        emit(setup=w.name, samples=a.samples, log2=a.log2, filters=a.filters, columns=cols, span=int(span), row_bytes=int(row_bytes),
             build_s=round(time.perf_counter() - t0, 1))
        T = ka.SEARCH_TIMING
        fs = ka.FilterSet.from_columns(g, cols)
        bits = fs.bit_counts()
        # (a)'s queries: random sequences whose k-mer positions number what the filters have set rows
        rng = np.random.default_rng(99)
        b = ka.Batch(ctx, [synth._rand_seq(rng, int(n) + w.kmer_len - 1) for n in bits])
        out_a = torch.empty((a.filters, span), dtype=torch.int32, device="cuda:%d" % ctx.device)
        out_b = torch.empty((a.filters, span), dtype=torch.int32, device="cuda:%d" % ctx.device)
        nk = torch.zeros((a.filters,), dtype=torch.int32, device="cuda:%d" % ctx.device)

        def run_a():
            return ka.search_scores_device(g, b, out_a, nk, flags=T)

        def run_b():
            return ka.search_filter_scores_device(g, fs, out_b, flags=T)

        # ---- exactness first ------------------------------------------------------------------------------------------------
        rb = run_b()
        got = out_b.cpu().numpy().view(np.uint32)
        own = [int(got[i, c]) for i, c in enumerate(cols)]
        col_bits = g.column_bits()
        assert own == bits.tolist() == [int(col_bits[c]) for c in cols], (own, bits.tolist())
        emit(check="cell (i, own column) == filter bits == column bits", bits=bits.tolist(), kernel=rb.kernel, equal=True)
        ra = run_a()
        rows_a = nk.cpu().numpy().view(np.uint32).astype(np.int64)
        rows_b = bits.astype(np.int64)

        # ---- timing: (a), (b), (c) alternating ------------------------------------------------------------------------------
        ms = {"a": [], "b": [], "c": []}
        for rep in range(a.warmup + a.reps):
            ra = run_a()
            rb = run_b()
            t1 = time.perf_counter()
            tmp = ka.FilterSet.from_columns(g, cols)
            dt = (time.perf_counter() - t1) * 1e3
            tmp.close()
            if rep >= a.warmup:
                ms["a"].append(float(ra.kernel_ms))
                ms["b"].append(float(rb.kernel_ms))
                ms["c"].append(dt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()}
        gbps = {"a": int(rows_a.sum()) * row_bytes / (med["a"] * 1e-3) / 1e9, "b": int(rows_b.sum()) * row_bytes / (med["b"] * 1e-3) / 1e9}
        emit(run="(a) search_scores_device, sequence batch", kernel=ra.kernel, rows=rows_a.tolist(), kernel_ms=round(med["a"], 4),
             spread=round(spread["a"], 4), reps=a.reps, all_ms=[round(x, 4) for x in ms["a"]], gbps=round(gbps["a"], 1))
        emit(run="(b) search_filter_scores_device, planted columns", kernel=rb.kernel, rows=rows_b.tolist(), kernel_ms=round(med["b"], 4),
             spread=round(spread["b"], 4), reps=a.reps, all_ms=[round(x, 4) for x in ms["b"]], gbps=round(gbps["b"], 1))
        ratio = gbps["b"] / gbps["a"]
        emit(expectation="(b) >= 0.95 (a), algorithmic bytes per second", b_over_a=round(ratio, 4), met=bool(ratio >= 0.95),
             rows_b_over_rows_a=round(float(rows_b.sum()) / float(rows_a.sum()), 4), same_kernels=(ra.kernel == rb.kernel))
        # ---- (c) against the streaming probe: one 64-byte sector per row and column --------------------------------------------
        stream = g.stream_read_gbps(min(g.device_bytes, 8 << 30), 3)
        implied_ms = a.filters * (1 << a.log2) * 64 / (stream * 1e9) * 1e3
        emit(run="(c) FilterSet.from_columns (extraction, wall)", wall_ms=round(med["c"], 3), spread=round(spread["c"], 4),
             all_ms=[round(x, 3) for x in ms["c"]], stream_probe_gbps=round(stream, 1), sector_bytes=64,
             implied_ms=round(implied_ms, 3), wall_over_implied=round(med["c"] / implied_ms, 2),
             extraction_over_one_search=round(med["c"] / med["b"], 3))
        fs.close()
        b.close()


if __name__ == "__main__":
    main()
