#!/usr/bin/env python3
"""The nearest-neighbour lists (kwage_group_column_neighbors) measured beside what there was before them, on one box in
one process: one resident group of 2^L rows and 8192 random columns at density 1/4 (rows 1 KiB apart), every column's 10
best partners by Jaccard index, itself left out.

  neighbours   Group.column_neighbors(10, skip_self=True) over all columns, at four values of the knob
               neighbors_strip_bytes: 16 MiB, 64 MiB, 256 MiB and 1 GiB -- strips of 512, 2048, 8192 and 8192 entries (a
               row of cells is 32 KiB here, so the two largest both make one strip: 16 MiB is there to tell a small
               budget from the default)
  before       Group.column_overlaps of all columns (the symmetric form) into an n x n tensor, then on that tensor the
               Jaccard index in float64 and a stable torch.sort of every row, descending

Each side runs in a context of its own, so that what the context's pool holds afterwards is what the call took at its
peak: free device memory before the group's first call minus free memory after it (for `before` plus torch's own peak,
which holds the n x n cells, the doubles and the sort's outputs).  Per side: the kernels' HIP-event time of --repeat
calls after one untimed call; for the neighbours the overlap kernels alone on the same strips' shape (column_overlaps in
the a x b form, timed the same way) and from it the select stage's share of the call; the wall time of a call.  The two
answers are compared: rows whose 10 indices agree (they may differ where doubles tie and fractions do not).

    python tools/neighbors_bench.py [--log2 20] [--repeat 3] [--k 10]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (a one-shot program: no second candidate block for the matrix, whose release costs seconds -- kwage_amd.h, kwage_group_placement)
os.environ.setdefault("KWAGE_GROUP_PLACEMENT_PROBE", "0")
import kwage_amd as ka

ap = argparse.ArgumentParser()
ap.add_argument("--log2", type=int, default=20)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--k", type=int, default=10)
args = ap.parse_args()
L, K, NH, CAP = args.log2, 31, 1, 8192
STRIPS = (16 << 20, 64 << 20, 256 << 20, 1 << 30)


def group_of(ctx):
    g = ka.Group(ctx, K, NH, L, CAP)
    assert g.add_random_columns(CAP, 7, 64) == 0
    g.finalize()
    return g


def neighbours(strip_bytes):
    import torch
    with ka.Context(0) as ctx:
        g = group_of(ctx)
        try:
            with ctx.tuning(neighbors_strip_bytes=strip_bytes):
                torch.cuda.synchronize()
                free0 = ctx.mem_info()[0]
                rec, cnt, st = g.column_neighbors(args.k, skip_self=True)           # (untimed: the first launch loads the code object)
                torch.cuda.synchronize()
                pool = free0 - ctx.mem_info()[0] - rec.numel() * 4 - cnt.numel() * 4
                ms, wall = [], []
                for _ in range(args.repeat):
                    t0 = time.perf_counter()
                    rec, cnt, st = g.column_neighbors(args.k, skip_self=True, timing=True)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(st["kernel_ms"])
                # the overlap kernels alone, strip by strip of the same shape
                e = int(st["strip_entries"])
                out = torch.empty((e, g.column_span), dtype=torch.int32, device="cuda")
                cols = np.arange(g.column_span)
                g.column_overlaps(cols[:e], g, None, out=out)
                overlap = []
                for _ in range(args.repeat):
                    total = 0.0
                    for first in range(0, g.column_span, e):
                        part = cols[first:first + e]
                        total += g.column_overlaps(part, g, None, out=out[:len(part)], timing=True)[1]["kernel_ms"]
                    overlap.append(total)
            best, best_overlap = min(ms), min(overlap)
            print("neighbours  neighbors_strip_bytes %4d MiB  strips=%d of %d entries  tiles=%d  records=%d  %s  kernel ms %s  (overlap kernels alone %s -> the select "
                  "stage's share %.2f)  wall ms %s  pool %.1f MB + result %.2f MB"
                  % (strip_bytes >> 20, st["strips"], st["strip_entries"], st["tiles"], st["records"], st["kernel"], " ".join("%.3f" % x for x in ms),
                     " ".join("%.3f" % x for x in overlap), max(0.0, 1.0 - best_overlap / best), " ".join("%.1f" % x for x in wall), pool / 1e6,
                     (rec.numel() + cnt.numel()) * 4 / 1e6), flush=True)
            return rec[:, :, 0].cpu().numpy()
        finally:
            g.close()


def before():
    import torch
    with ka.Context(0) as ctx:
        g = group_of(ctx)
        try:
            n = g.column_span

            def answer(timing):
                cells, st = g.column_overlaps(timing=timing)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                sh = cells.to(torch.float64)
                bits = torch.diagonal(sh)
                union = bits[:, None] + bits[None, :] - sh
                jac = torch.where(union > 0, sh / union.clamp(min=1), torch.zeros_like(sh))
                jac.fill_diagonal_(-1.0)                                        # (the column itself left out)
                order = torch.sort(jac, dim=1, descending=True, stable=True).indices[:, :args.k]
                ev[1].record()
                torch.cuda.synchronize()
                return order, st, ev[0].elapsed_time(ev[1])

            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            free0 = ctx.mem_info()[0]
            answer(False)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            torch.cuda.empty_cache()
            pool = free0 - ctx.mem_info()[0]
            ms, sort_ms, wall = [], [], []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                order, st, t_sort = answer(True)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(st["kernel_ms"])
                sort_ms.append(t_sort)
            print("before      column_overlaps %d x %d (symmetric, tiles=%d, %s) kernel ms %s  + Jaccard in float64 and a stable torch.sort per row, device ms %s  "
                  "wall ms %s  pool and caches %.1f MB + torch's peak %.1f MB"
                  % (n, n, st["tiles"], st["kernel"], " ".join("%.3f" % x for x in ms), " ".join("%.3f" % x for x in sort_ms), " ".join("%.1f" % x for x in wall),
                     pool / 1e6, peak / 1e6), flush=True)
            return order.cpu().numpy()
        finally:
            g.close()


with ka.Context(0) as ctx0:
    print("device: " + ";".join("%s=%s" % kv for kv in ctx0.fingerprint().items()))
    warm = ka.Group(ctx0, K, NH, 10, CAP)             # (a kernel's first launch loads its code object: not timed)
    warm.add_random_columns(CAP, 1, 64)
    warm.finalize()
    warm.column_neighbors_host(2, [0, 1])
    warm.close()
print("group: 2^%d rows, %d random columns at density 1/4, k = %d, Jaccard, the column itself left out" % (L, CAP, args.k), flush=True)
lists = [neighbours(s) for s in STRIPS]
for other in lists[1:]:
    assert np.array_equal(lists[0], other), "the lists depend on the strips"
old = before()
same = int((old == lists[0].astype(np.int64)).all(axis=1).sum())
print("rows whose %d neighbours agree between the two answers: %d of %d" % (args.k, same, len(old)), flush=True)
