"""The host-side plan of the builder and the re-pack (kwage_amd/csrc/build_plan.hpp: rows per chunk, chunks, the stride of
the filters in the device's input block), built with g++ -fsanitize=address,undefined as a stand-alone program
(tests/sanitize/build_plan_sanitize.cpp) that reads a file of cases and prints each plan.  Two sets of cases: the plan at
sizes no GPU test can afford (2048 filters of 2^23 bits, one filter of 2^32 bits) and at the shapes the GPU tests of
tests/test_builder.py run, and the plan's invariants over a few thousand pseudo-random inputs.  CPU only: no device is
touched, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")
MIB = 1 << 20
DEFAULT = 256 * MIB
FLOOR = 1024


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("build_plan")
    exe = str(tmp / "build_plan_sanitize")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + csrc, os.path.join(ROOT, "tests", "sanitize", "build_plan_sanitize.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]

    def plan(cases, name):
        """cases: ("B", budget, n, filter_len, pad) or ("R", budget, nrows, dst_words, max_width) -> [{field: int}] in order."""
        path = str(tmp / name)
        with open(path, "w") as f:
            f.write("".join("%d %s\n" % (i, " ".join(map(str, c))) for i, c in enumerate(cases)))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr or "ReserveShadowMemoryRange failed" in r.stderr):
            pytest.skip("the sanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0][:200])
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
        assert "no report" in r.stdout and not any(x in r.stderr for x in REPORTS), r.stderr[-4000:]
        out = {}
        for line in r.stdout.splitlines():
            if line.startswith("case "):
                w = line.split()
                out[int(w[1])] = {k: int(v) for k, v in (x.split("=", 1) for x in w[2:])}
        assert sorted(out) == list(range(len(cases)))
        return [out[i] for i in range(len(cases))]

    return plan


def B(n, L, budget=0, pad=-1):
    return ("B", budget, n, 1 << L, pad)


def test_build_plan_at_pinned_sizes(planner):
    """(n filters, L) -> (chunk_rows, in_stride, chunks).  The first four at the default budget: what kwage_build_db has
    always done.  One filter of 2^32 bits takes 16 chunks, not the two its 512 MiB of input alone would ask for: the
    output of a chunk is rows x 1 byte here, and 2^28 rows are the most that keep it within 256 MiB."""
    cases = [
        (B(2048, 23), (1 << 20, 131072 + 256, 8)),              # 2^20 rows: input and output exactly 256 MiB; 512 units -> 513
        (B(2048, 20), (1 << 20, 131072 + 256, 1)),
        (B(2049, 20), (1 << 19, 65536 + 256, 2)),               # one filter more: the input no longer fits
        (B(1, 32), (1 << 28, (1 << 25) + 256, 16)),
        (B(1, 3), (8, 256, 1)), (B(3, 0), (1, 256, 1)),         # filters shorter than the floor: whole, one 256-byte unit apart
        (B(2048, 23, budget=DEFAULT), (1 << 20, 131072 + 256, 8)),
        # the shapes of tests/test_builder.py's multi-chunk cases
        (B(1025, 13, budget=256 << 10), (1024, 256, 8)),        # the floor: the output of 1024 rows (129 KiB) would fit, 2048 not
        (B(300, 12, budget=64 << 10), (1024, 256, 4)),
        (B(2500, 11, budget=1 << 10), (1024, 256, 2)),          # the floor holds although neither buffer fits
        (B(1025, 13, budget=256 << 10, pad=4), (1024, 132, 8)),
        (B(1025, 13, budget=256 << 10, pad=0), (1024, 128, 8)), (B(1025, 13, budget=256 << 10, pad=7), (1024, 132, 8)),
        (B(5, 1, pad=0), (2, 4, 1)),                            # never below the chunk itself, in whole dwords
        (B(1300, 12), (4096, 768, 1)),                          # 512 bytes = 2 units -> 3
        (B(64, 14), (16384, 2048 + 256, 1)), (B(64, 13), (8192, 1024 + 256, 1)), (B(64, 11), (2048, 256, 1)), (B(64, 12), (4096, 768, 1)),
    ]
    got = planner([c for c, _ in cases], "pinned_build.txt")
    for (c, want), g in zip(cases, got):
        assert (g["chunk_rows"], g["in_stride"], g["chunks"]) == want, (c, g)


def test_repack_plan_at_pinned_sizes(planner):
    cases = [
        (("R", 0, 1 << 20, 64, 256), (1 << 20, 1)),             # 2048 columns x 2^20 rows: 256 MiB exactly
        (("R", 0, 1 << 20, 65, 256), (1 << 19, 2)),
        (("R", 0, 1 << 23, 64, 256), (1 << 20, 8)),
        (("R", 0, 1 << 20, 64, 257), (1 << 19, 2)),             # the widest source decides
        (("R", 4 << 10, 1 << 10, 8, 17), (128, 8)),             # tests/test_builder.py: 236 columns -> 30 bytes -> 8 dwords
        (("R", 1, 1 << 10, 8, 17), (1, 1024)),                  # the floor: one row per chunk
        (("R", 31, 1 << 10, 8, 17), (1, 1024)), (("R", 32, 1 << 10, 8, 17), (1, 1024)), (("R", 64, 1 << 10, 8, 17), (2, 512)),
        (("R", 0, 1, 1, 1), (1, 1)),
        (("R", 1 << 10, 1000, 8, 17), (31, 33)),                # not a power of two: the last chunk takes the 8 rows left
    ]
    got = planner([c for c, _ in cases], "pinned_repack.txt")
    for (c, want), g in zip(cases, got):
        assert (g["chunk_rows"], g["chunks"]) == want, (c, g)


def test_plan_invariants_over_random_inputs(planner):
    rng = np.random.default_rng(20240911)
    budgets = [0, 1, 1023, 1 << 10, 4 << 10, 64 << 10, 256 << 10, MIB, 100 * MIB + 1, DEFAULT - 1, DEFAULT, DEFAULT + 1, 1 << 32, 1 << 40]
    ns = [1, 2, 7, 8, 9, 64, 300, 1024, 1025, 2047, 2048, 2049, 2500, 65536, 10 ** 6, (1 << 32) - 1]
    build, repack = [], []
    for i in range(3000):
        budget = int(rng.choice(budgets)) if i % 2 else int(np.exp(rng.uniform(0, np.log(1 << 40))))
        n = int(rng.choice(ns)) if i % 3 else int(np.exp(rng.uniform(0, np.log((1 << 32) - 1))))
        L = int(rng.integers(0, 33))
        pad = -1 if rng.random() < 0.7 else int(rng.choice([0, 1, 3, 4, 5, 255, 256, 260, 1 << 20]))
        build.append(B(n, L, budget, pad))
        nrows = 1 << L if rng.random() < 0.8 else int(np.exp(rng.uniform(0, np.log(1 << 32))))
        slice_bytes = (n + 7) // 8
        repack.append(("R", budget, nrows, (slice_bytes + 3) // 4, int(rng.integers(1, slice_bytes + 1))))
    for (_, budget, n, flen, pad), g in zip(build, planner(build, "grid_build.txt")):
        what = (budget, n, flen, pad, g)
        budget = budget or DEFAULT
        rows, stride, chunks, slice_bytes = g["chunk_rows"], g["in_stride"], g["chunks"], (n + 7) // 8
        fits = lambda r: r // 8 * n <= budget and r * slice_bytes <= budget
        assert rows & (rows - 1) == 0 and rows >= min(FLOOR, flen) and flen % rows == 0 and rows <= flen, what
        assert chunks * rows == flen, what
        assert fits(rows) or rows == min(FLOOR, flen), what                  # within the budget unless the floor holds
        assert rows == flen or not fits(2 * rows), what                      # and no smaller than the budget asks for
        chunk_bytes = (rows + 7) // 8
        assert stride >= chunk_bytes and stride % 4 == 0, what
        if pad < 0:
            assert stride % 256 == 0 and (stride // 256) % 2 == 1 and stride - chunk_bytes < 512, what
        else:
            assert stride == (chunk_bytes + 3) // 4 * 4 + pad // 4 * 4, what
    for (_, budget, nrows, dst_words, max_width), g in zip(repack, planner(repack, "grid_repack.txt")):
        what = (budget, nrows, dst_words, max_width, g)
        budget = budget or DEFAULT
        rows, chunks = g["chunk_rows"], g["chunks"]
        fits = lambda r: r * dst_words * 4 <= budget and r * max_width <= budget
        assert 1 <= rows <= nrows and (chunks - 1) * rows < nrows <= chunks * rows, what      # the chunks cover the rows exactly
        assert fits(rows) or rows == 1, what
        assert rows == nrows or not fits(2 * rows + 1), what                 # (halving rounds down: 2 rows + 1 was the step before)
