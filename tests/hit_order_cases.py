"""Run tables and raw hit lists for order_hits_by_runs (kwage_amd/csrc/hit_sort.hip), with the numpy reference of what it
must make of them.  A table entry is `first << 16 | records`: a run of `records` hit records that lies at slot `first` of
the raw list, already ascending; the entries are in key order, so the ordered list is the runs in table order.

Every case names the edge of hit_sort.hip it is there for; tests/test_hit_order_cases.py recomputes that property from
the table (no GPU), tests/test_gpu_hit_order.py feeds every case to the device code.

What the cases never do: claim more records than the list holds (the compact run lists are sized for
min(n_runs, n_hits) + 1 runs: the device code could write outside them, and the engine cannot make such a table), and
n_hits = 0 (the engine never calls with it)."""
import functools
import os
import subprocess
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_driver(out_dir):
    """hit_order_driver from its own file + hit_sort.hip + host.cpp (kwage::fail), with the Makefile's flags: the
    sources, not libkwage_amd.so -- order_hits_by_runs is no ABI symbol.  host.cpp is compiled on its own, as the Makefile
    does: with `-x c++` on its line hipcc leaves --offload-arch out and builds the device code for its default target."""
    exe, host_o = os.path.join(str(out_dir), "hit_order_driver"), os.path.join(str(out_dir), "host.o")
    flags = ["-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    driver = os.path.join(ROOT, "tests", "device", "hit_order_driver.hip")
    # (the object comes first: the `-x hip` that hipcc puts in front of a .hip file holds for everything behind it)
    for cmd in ([HIPCC] + flags + ["-x", "c++", "-c", os.path.join(CSRC, "host.cpp"), "-o", host_o],
                [HIPCC, "--offload-arch=gfx950"] + flags + [host_o, driver, os.path.join(CSRC, "hit_sort.hip"), "-o", exe, "-lz"]):
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
    # the device code is in the program, and for this GPU (a program without it dies at its first launch)
    image = open(exe, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in image and b"amdgcn-amd-amdhsa--gfx906" not in image, "no gfx950 code object in " + exe
    return exe


# hit_sort.hip's constants, restated
ENTRIES_PER_THREAD = 4
ENTRIES_PER_BLOCK = 1024      # table entries per workgroup of run_block_sums / run_compact
SCAN_THREADS = 1024           # threads of the one workgroup of run_scan_sums
COPY_CHUNK = 2048             # ordered records per workgroup of run_copy
MAX_RUN = 0xFFFF              # the length field's 16 bits

HIT_WORDS = 3                 # kwage_hit: query, column, num_match
SENTINEL = 0xA5               # the byte tests/device/hit_order_driver.hip fills the scratch block with
UNDER_CLAIM = 5


@dataclass(frozen=True)
class Case:
    name: str
    edge: str                 # which check of test_hit_order_cases.py applies
    table: np.ndarray         # uint64 [n_runs]
    n_hits: int
    want: tuple = ()          # parameters of that check


def lens_of(table):
    return (table & np.uint64(0xFFFF)).astype(np.int64)


def firsts_of(table):
    return (table >> np.uint64(16)).astype(np.int64)


def raw_list(n_hits):
    """uint32 [n_hits, 3], pairwise distinct: record i carries i and two mixed values of i."""
    i = np.arange(n_hits, dtype=np.uint64)
    out = np.empty((n_hits, HIT_WORDS), dtype=np.uint32)
    out[:, 0] = i
    out[:, 1] = ((i * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFFFFFF)
    out[:, 2] = ((i ^ (i >> np.uint64(3))) * np.uint64(40503) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    return out


def reference(table, raw):
    """(total, ordered[:total]) -- the runs in table order."""
    lens = lens_of(table)
    first = firsts_of(table)
    nz = lens > 0
    to = np.cumsum(lens) - lens
    total = int(lens.sum())
    return total, raw[np.repeat(first[nz] - to[nz], lens[nz]) + np.arange(total)]


def reference_loop(table, raw):
    """The same, one run at a time."""
    out = []
    for e in table.tolist():
        n, first = e & 0xFFFF, e >> 16
        out.extend(raw[first + j] for j in range(n))
    return len(out), np.array(out, dtype=np.uint32).reshape(-1, HIT_WORDS)


def pack(lens, rng):
    """The table of runs of these lengths (0: an empty entry), laid into the raw list in a shuffled order without gaps:
    what the kernels' atomic reservations of hit slots produce."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.ndim == 1 and lens.size and 0 <= lens.min() and lens.max() <= MAX_RUN
    nz = np.flatnonzero(lens)
    order = rng.permutation(nz)
    first = np.zeros(lens.size, dtype=np.int64)
    first[order] = np.cumsum(lens[order]) - lens[order]
    table = np.where(lens > 0, (first << 16) | lens, 0).astype(np.uint64)
    return table, int(lens.sum())


def _lens_summing_to(n_hits, rng, max_len=64):
    out = []
    left = n_hits
    while left:
        n = min(left, int(rng.integers(1, max_len + 1)))
        out.append(n)
        left -= n
    return np.array(out, dtype=np.int64)


def _sprinkle(n_runs, rng, share, max_len):
    """n_runs entries, about `share` of them runs of 1 .. max_len records."""
    lens = rng.integers(1, max_len + 1, size=n_runs)
    lens[rng.random(n_runs) >= share] = 0
    return lens


def _tail(n_runs):
    def build(rng):
        lens = rng.integers(1, 65, size=n_runs)
        if n_runs > 8:
            lens[rng.random(n_runs) < 0.25] = 0
            lens[-1] = 3         # the entry the tails are about is not empty
        return Case("tail-%d" % n_runs, "n_runs", *pack(lens, rng), want=(n_runs,))
    return build


def _scan(nblocks, per, extra):
    def build(rng):
        n_runs = (nblocks - 1) * ENTRIES_PER_BLOCK + extra
        lens = _sprinkle(n_runs, rng, 0.01, 32)
        lens[-1] = 9             # the last block's sum, in the last scan thread that has a stretch
        return Case("scan-%d-blocks" % nblocks, "scan", *pack(lens, rng), want=(nblocks, per))
    return build


def _blocks(name, edge, n_blocks, extra, empty_blocks, last_entry=None):
    def build(rng):
        n_runs = n_blocks * ENTRIES_PER_BLOCK + extra
        lens = _sprinkle(n_runs, rng, 0.3, 48)
        for b in empty_blocks(n_blocks):
            lens[b * ENTRIES_PER_BLOCK:(b + 1) * ENTRIES_PER_BLOCK] = 0
        if last_entry is not None:
            lens[-1] = last_entry
        return Case(name, edge, *pack(lens, rng))
    return build


def _late_start(rng):
    lens = _sprinkle(6 * ENTRIES_PER_BLOCK + 77, rng, 0.3, 48)
    lens[:4096 + 301] = 0
    return Case("first-run-beyond-4096", "late_start", *pack(lens, rng))


def _all_ones(rng):
    lens = np.ones(3 * COPY_CHUNK + 1 + 500, dtype=np.int64)
    lens[rng.choice(lens.size, 500, replace=False)] = 0
    return Case("all-runs-of-one", "all_ones", *pack(lens, rng))


def _longest(rng):
    lens = np.concatenate([np.ones(1000, np.int64), [MAX_RUN], np.ones(3000, np.int64)])
    return Case("longest-run", "longest", *pack(lens, rng))


def _kernel_lengths_lens(rng):
    lens = _sprinkle(3000, rng, 0.5, 64)
    where = rng.choice(lens.size - 1, 26, replace=False)
    lens[where[:20]] = 8192
    lens[where[20:]] = 32768
    lens[-1] = 37                # (the entry the under-claiming copy of this case shortens)
    return lens


def _kernel_lengths(rng):
    return Case("kernel-lengths", "kernel_lengths", *pack(_kernel_lengths_lens(rng), rng))


def _chunk(n_hits):
    def build(rng):
        lens = _lens_summing_to(n_hits, rng)
        spread = np.zeros(2 * lens.size + 3, dtype=np.int64)
        spread[rng.choice(spread.size, lens.size, replace=False)] = 1
        spread[spread > 0] = lens
        return Case("hits-%d" % n_hits, "n_hits", *pack(spread, rng), want=(n_hits,))
    return build


def _under_claim(name, base):
    def build(rng):
        c = base(rng)
        table = c.table.copy()
        last = int(np.flatnonzero(lens_of(table))[-1])
        assert int(lens_of(table)[last]) > UNDER_CLAIM, (c.name, "the last run is too short to lose %d records" % UNDER_CLAIM)
        table[last] -= np.uint64(UNDER_CLAIM)
        return Case(name, "under_claim", table, c.n_hits, want=(c.n_hits - UNDER_CLAIM,))
    return build


def _hits_2049_long_tail(rng):
    lens = np.concatenate([_lens_summing_to(COPY_CHUNK - 10, rng), [0, 0, 11]])
    return Case("hits-2049-last-run-of-11", "n_hits", *pack(lens, rng), want=(COPY_CHUNK + 1,))


_BUILDERS = (
    [_tail(n) for n in (1, 3, 4, 5, 1023, 1024, 1025)]
    + [_scan(1024, 1, 1021), _scan(1025, 2, 5), _scan(2049, 3, 7)]
    + [_blocks("first-block-empty", "first_block_empty", 5, 13, lambda n: [0]),
       _blocks("last-block-empty", "last_block_empty", 5, 13, lambda n: [n]),          # (the partial block behind the five)
       _blocks("every-other-block-empty", "alternate_blocks_empty", 9, 0, lambda n: range(1, n, 2)),
       _late_start,
       _blocks("last-entry-not-empty", "last_entry", 3, 1, lambda n: [], last_entry=21)]
    + [_all_ones, _longest, _kernel_lengths]
    + [_chunk(n) for n in (1, 2047, 2048, 2049)]
    + [_under_claim("under-claim-kernel-lengths", _kernel_lengths),
       _under_claim("under-claim-hits-2049", _hits_2049_long_tail)]       # the table's total ends one chunk earlier than the list
)


@functools.lru_cache(maxsize=None)
def _built():
    out = {}
    for k, build in enumerate(_BUILDERS):
        c = build(np.random.default_rng(20240 + k))       # fixed seeds: the cases are the same in every run
        assert c.name not in out, c.name
        c.table.setflags(write=False)
        out[c.name] = c
    return out


def names():
    return list(_built())


def case(name):
    return _built()[name]


SMALL = 40000     # cases with at most this many records are also checked against reference_loop
