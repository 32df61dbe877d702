#!/usr/bin/env python3
"""Dense score search timings at the C2 shape (100 k samples x 2^23-bit filters, 1 k x 1 kb queries, 1 hash;
kwage_amd/synth.py), in one process on one box, the four runs alternating repetition by repetition:

  (a) kwage_search at t = 0.8 with the tiled count_kernel forced (knob count_walk = 0): the yardstick
  (b) search_topk k = 10 at t = 0.8: what a different epilogue on the same tile loop is known to cost
  (c) search_scores_device with each store epilogue (knob scores_form: 0 = a KiB of consecutive cells per store
      instruction, 1 = every lane its own 512-byte run)
  (d) the low-threshold route the dense search replaces: kwage_search at t = 1e-4 (every column a hit) copied back and
      re-densified on the host, wall time against (c)'s wall time

Kernel times are HIP-event times of the search stage, the median of --reps repetitions after --warmup; the spread is
(max - min) / median over the repetitions.  The dense search reads what (a) reads (algorithmic_bytes) and writes
queries x span x 4 bytes on top, so the expectation tested is

    (c)/(a)  <=  (b)/(a) + written/read + 0.05

Before timing, a sample of rows of (c) is checked against (a)'s hit list: the columns at or above the floor 0.8 n and
their scores, exactly.  One JSON line per record, each with the device's fingerprint.
   python tools/bench_scores.py [--log2 23] [--samples 100000] [--reps 7] [--warmup 2] [--no-low]"""
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

FORMS = {0: "wave (1 KiB per store)", 1: "lane (512-byte runs)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=23)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-rows", type=int, default=24)
    ap.add_argument("--no-low", action="store_true", help="skip the low-threshold route (a 100 M-record hit list at C2)")
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
        emit(setup=w.name, samples=a.samples, log2=a.log2, queries=a.queries, span=int(span), build_s=round(time.perf_counter() - t0, 1))
        T = ka.SEARCH_TIMING
        out = torch.empty((n, span), dtype=torch.int32, device="cuda:%d" % ctx.device)

        def run_a():
            with ctx.tuning(count_walk=0):
                return g.search(b, 0.8, T)

        def run_b():
            return ka.search_topk(g, b, 10, 0.8, T)

        def run_c(form):
            with ctx.tuning(scores_form=form):
                return ka.search_scores_device(g, b, out, flags=T)

        # ---- exactness first: sampled rows of (c), each form, against (a)'s hit list at the floor 0.8 n ----------------------
        ref = run_a()
        assert ref.search_kernel.startswith("count_kernel<"), ref.search_kernel
        rows = sorted(set(np.linspace(0, n - 1, a.check_rows).astype(int).tolist()))
        hq = ref.hits["query"]
        for form in FORMS:
            out.fill_(-1)
            res = run_c(form)
            for q in rows:
                row = out[q].cpu().numpy().view(np.uint32)
                mine = np.flatnonzero(row >= max(int(ref.query_threshold[q]), 1))
                lo, hi = np.searchsorted(hq, q, "left"), np.searchsorted(hq, q, "right")
                theirs = ref.hits[lo:hi]
                assert np.array_equal(mine, theirs["column"]) and np.array_equal(row[mine], theirs["num_match"]), (form, q)
            emit(check="rows of search_scores_device against kwage_search t=0.8", form=FORMS[form], rows=len(rows), kernel=res.kernel, equal=True)

        # ---- timing: (a), (b), (c) x forms alternating ------------------------------------------------------------------------
        runs = [("a", run_a, lambda r: r.search_kernel_ms), ("b", run_b, lambda r: r.search_kernel_ms)] + \
               [("c%d" % f, (lambda f=f: run_c(f)), lambda r: r.kernel_ms) for f in FORMS]
        ms = {name: [] for name, _, _ in runs}
        wall = {name: [] for name, _, _ in runs}
        kernels = {}
        for rep in range(a.warmup + a.reps):
            for name, fn, get in runs:
                t1 = time.perf_counter()
                r = fn()
                dt = (time.perf_counter() - t1) * 1e3
                kernels[name] = r.search_kernel if hasattr(r, "search_kernel") else r.kernel
                if rep >= a.warmup:
                    ms[name].append(float(get(r)))
                    wall[name].append(dt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()}
        read = int(ref.algorithmic_bytes)
        written = int(n) * int(span) * 4
        labels = {"a": "kwage_search t=0.8 count_kernel", "b": "search_topk k=10 t=0.8"}
        labels.update({"c%d" % f: "search_scores_device, " + FORMS[f] for f in FORMS})
        for name, _, _ in runs:
            emit(run=labels[name], kernel=kernels[name], kernel_ms=round(med[name], 4), spread=round(spread[name], 4),
                 wall_ms=round(statistics.median(wall[name]), 3), reps=a.reps, all_ms=[round(x, 4) for x in ms[name]],
                 gbps=round((read + (written if name.startswith("c") else 0)) / (med[name] * 1e-3) / 1e9, 1))
        best = min(FORMS, key=lambda f: med["c%d" % f])
        bound = med["b"] / med["a"] + written / read + 0.05
        for f in FORMS:
            ratio = med["c%d" % f] / med["a"]
            emit(expectation="(c)/(a) <= (b)/(a) + written/read + 0.05", form=FORMS[f], faster_form=(f == best),
                 c_over_a=round(ratio, 4), b_over_a=round(med["b"] / med["a"], 4), written_over_read=round(written / read, 4),
                 bound=round(bound, 4), met=bool(ratio <= bound), missed_by=round(max(0.0, ratio - bound), 4),
                 spread_a=round(spread["a"], 4), spread_b=round(spread["b"], 4), spread_c=round(spread["c%d" % f], 4),
                 bytes_read=read, bytes_written=written)

        # ---- (d) the low-threshold route: hit list of every (query, column) pair, copied back, re-densified on the host ----------
        if not a.no_low:
            def low():
                r = g.search(b, 1e-4)
                m = np.zeros((n, span), dtype=np.uint32)
                m[r.hits["query"], r.hits["column"]] = r.hits["num_match"]
                return r, m
            low()
            walls = []
            for _ in range(max(2, a.reps // 3)):
                t1 = time.perf_counter()
                r, m = low()
                walls.append((time.perf_counter() - t1) * 1e3)
            dense = out.cpu().numpy().view(np.uint32)              # (the last timed run's matrix)
            nz = dense > 0
            agree = bool(np.array_equal(m[nz], dense[nz])) if r.hits.size == int(n) * int(g.num_columns) else None
            c_wall = statistics.median(wall["c%d" % best])
            emit(run="low-threshold route t=1e-4 + host densify", kernel=r.search_kernel, wall_ms=round(statistics.median(walls), 1),
                 hits=int(r.hits.size), hit_bytes=int(r.hits.size) * 12, scores_wall_ms=round(c_wall, 3),
                 wall_ratio_d_over_c=round(statistics.median(walls) / c_wall, 1), nonzero_cells_equal=agree)


if __name__ == "__main__":
    main()
