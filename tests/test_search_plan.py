"""The host-side plan of the threshold search's gather stage (kwage_amd/csrc/search_plan.hpp: which form runs, its template
integers, segments, launch shapes, list capacities, the truncated walk's tables, the reported name), built with
g++ -fsanitize=address,undefined as a stand-alone program (tests/sanitize/search_plan_sanitize.cpp) that reads a file of
cases and prints each plan.  Two sets of cases: every row of search_shapes.CASES (and of search_holes.WIDE_CASES) on a device
of 256 CUs must plan the name the GPU test asserts, and a few thousand pseudo-random inputs must keep the plan's invariants.  CPU only: no device
is touched, nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import search_shapes as ss

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")
NCU = 256
EE = ss.EE
FORMS = ("AND_NARROW", "AND_SCREEN", "AND_BAND_WALK", "AND_WALK", "AND_TILED",
         "COUNT_SCREEN", "COUNT_WALK_TRUNC", "COUNT_WALK", "COUNT_NARROW", "COUNT_TILED")
# each knob's values in the tests (search_shapes.CASES, the variants of test_gpu_search_shapes.py); absent: its default
KNOB_TEST_VALUES = {
    "walk": (0,), "walk_min_rows": (1,), "walk_min_kib": (1,), "walk_bands": (0, 3, 5), "walk_bands_min_gib": (0,), "walk_waves": (5, 3001),
    "and_vec": (1, 2, 4), "force_segs": (1, 2, 3, 7, 100), "refine_unroll": (16,), "refine_list_cap": (5,), "refine_seg_rows": (8, 120),
    "refine_static": (0,), "count_screen_min_tiles": (1, 1 << 30), "count_walk_min_rows": (1,), "count_walk_waves": (7, 3001),
    "narrow": (0,), "ee_refine": (0,), "count_trunc": (0,), "count_walk": (0,), "and_wide": (0,), "walk_max_kib": (32,), "walk_tile_kib": (4,),
}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("search_plan")
    exe = str(tmp / "search_plan_sanitize")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "search_plan_sanitize.cpp"), "-o", exe, "-lz", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]

    def plan(cases, name):
        """cases: lists of fields (see case_line) -> {id: {field: value}} of the program's lines, after the sanitizer checks."""
        path = str(tmp / name)
        with open(path, "w") as f:
            f.write("".join("%d %s\n" % (i, c) for i, c in enumerate(cases)))
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
                out[int(w[1])] = dict(x.split("=", 1) for x in w[2:])
        assert sorted(out) == list(range(len(cases)))
        return out

    return plan


def case_line(ncu, stride, nrows, nh, density_max, t, flags, knobs, groups, alloc=None, mixes=0, blocks_per_cu=2):
    """One case of the program's input: the group's shape, the call, the knobs {name: value} and the batch as (count, positions) runs."""
    return " ".join(map(str, [ncu, stride, nrows, nh, nrows * stride if alloc is None else alloc, mixes, repr(float(density_max)), repr(float(np.float32(t))), flags,
                              blocks_per_cu, len(knobs)] + [x for kv in sorted(knobs.items()) for x in kv] + [len(groups)] + [x for g in groups for x in g]))


def runs_of(npos):
    """[(count, positions)] runs of a list of position counts."""
    out = []
    for n in npos:
        if out and out[-1][1] == n:
            out[-1][0] += 1
        else:
            out.append([1, n])
    return out


_batches = {}


def batch_runs(key):
    if key not in _batches:
        seqs, _ = ss.batch_seqs(key, NCU)
        _batches[key] = runs_of([max(len(s) - ss.K + 1, 0) for s in seqs])
    return _batches[key]


def test_every_case_plans_its_name(planner):
    """Every row of search_shapes.CASES, for every flag value it lists, at 256 CUs.  The truncated-walk rows are planned with
    the fill probability the GPU test draws the group with as the densest column's density, and again with 0.05 more: the
    sampled densest column of 8099 lies a few sigma (0.007 each at 4096 sampled rows) above the fill, never 0.05.  No row is
    left to the GPU test alone."""
    lines, want = [], []
    for ci, c in enumerate(ss.CASES):
        W, nh, L = ss.group_shape(c.group)
        stride = ((W + 7) // 8 + 127) // 128 * 128
        fill = 1.0 if c.group[0] == "count_dense" else ss.group_fill(c.group)
        for fl in c.flags:
            for dm in ((fill, fill + 0.05) if c.test == "count_walk_trunc" else (fill,)):
                lines.append(case_line(NCU, stride, 1 << L, nh, dm, c.t, fl, c.knobs, batch_runs(c.batch)))
                want.append((ci, c, fl, dm))
    got = planner(lines, "cases.txt")
    for i, (ci, c, fl, dm) in enumerate(want):
        assert got[i]["rc"] == "0" and got[i]["name"] == c.name, (c, fl, dm, got[i])
    assert {ci for ci, _, _, _ in want} == set(range(len(ss.CASES)))


def test_wide_count_cases_plan_their_names(planner):
    """The cases search_holes.py adds to the table, on the group of three KiB-steps: the same inputs as above, the truncated
    walk again at the fill and 0.05 above it."""
    import search_holes as sh
    lines, want = [], []
    for c in sh.WIDE_CASES:
        W, nh, L = ss.group_shape(c.group)
        fill = ss.group_fill(c.group)
        for fl in c.flags:
            for dm in ((fill, fill + 0.05) if c.test == "count_walk_trunc" else (fill,)):
                lines.append(case_line(NCU, sh.stride_bytes(W), 1 << L, nh, dm, c.t, fl, c.knobs, batch_runs(c.batch)))
                want.append((c, fl, dm))
    got = planner(lines, "wide.txt")
    assert len(want) >= 10
    for i, (c, fl, dm) in enumerate(want):
        assert got[i]["rc"] == "0" and got[i]["name"] == c.name and got[i]["chunks"] == "3", (c, fl, dm, got[i])


def test_plan_invariants_over_a_grid(planner):
    rng = np.random.default_rng(20240607)
    lines, inputs = [], []
    max_positions = (0, 1, 63, 64, 127, 128, 1023, 1024, 8192, 8193, 16383, 16384, 100000, (1 << 20) - 1, 1 << 20, (1 << 21) + 100)
    for i in range(4000):
        stride = 128 * int(rng.choice([1, 2, 3, 4, 5, 8, 13, 16, 24, 32, 40, 64, 100, 128, 129, 200, 256]))      # 128 B .. 32 KiB
        nq = int(rng.choice([1, 2, 3, 63, 64, 65, 300, 2047, 2048, 10000, 65535, 65536, 100000])) if i % 2 else int(np.exp(rng.uniform(0, np.log(100000))))
        mp = int(rng.choice(max_positions)) if i % 3 else int(np.exp(rng.uniform(0, np.log((1 << 21) + 100))))
        # the longest query first, then runs of shorter ones
        groups, left = [[1, mp]], nq - 1
        while left > 0:
            cnt = int(rng.integers(1, left + 1))
            groups.append([cnt, int(rng.integers(0, mp + 1)) if rng.random() < 0.7 else mp])
            left -= cnt
        knobs = {k: int(rng.choice(v)) for k, v in KNOB_TEST_VALUES.items() if rng.random() < 0.3}
        t = 1.0 if rng.random() < 0.5 else float(rng.choice([0.9, 0.8, 0.5, 0.05]))
        fl = int(rng.integers(0, 2))
        nh = int(rng.integers(1, 8))
        ncu = int(rng.choice([1, 64, 256, 304]))
        nrows = 1 << int(rng.integers(10, 24))
        lines.append(case_line(ncu, stride, nrows, nh, float(rng.uniform(0, 1)), t, fl, knobs, groups,
                               alloc=nrows * stride if rng.random() < 0.5 else 64 << 30, mixes=int(rng.integers(0, 2)), blocks_per_cu=int(rng.integers(1, 9))))
        inputs.append((stride, nq, mp, t, fl, nh, knobs))
    got = planner(lines, "grid.txt")
    names = set(ss.printable_names())
    seen = set()
    for i, (stride, nq, mp, t, fl, nh, knobs) in enumerate(inputs):
        g = {k: (int(v) if v.isdigit() else v) for k, v in got[i].items()}
        what = (lines[i][:300], got[i])
        tiles = nq * g["segs"] * g["chunks"]
        if g["rc"] != 0:
            assert tiles // 4 + 1 > 0x7FFFFFFF, what          # the one refusal the grid can reach
            continue
        form = FORMS[g["form"]]
        seen.add(form)
        # every template integer is an instantiated one: the name is one the ledger enumerates (FORMATS) ...
        assert g["name"] in names or (form == "COUNT_NARROW" and nh > 5), what
        if form == "COUNT_NARROW":        # (... this name prints the hash count unclamped: understood through launched())
            assert ss.launched(g["name"]), what
        assert form.startswith("AND") == (t == 1.0), what
        # 14-plane refine units never pair with fewer than 14 emit planes
        if form in ("COUNT_SCREEN", "COUNT_WALK_TRUNC") and g["up"] == 14:
            assert (g["planes"] if form == "COUNT_SCREEN" else g["tplanes"]) >= 14, what
        assert g["segs"] >= 1 and g["segs"] * g["seg_kmers"] >= mp, what
        if form == "COUNT_TILED" and g["segs"] > 1:
            assert 0 < g["partial_bytes"] == nq * g["segs"] * g["seg_planes"] * stride <= 1 << 30, what
        assert tiles // 4 + 1 <= 0x7FFFFFFF, what
        if nq > 65535:
            assert g["segs"] == 1, what
        assert g["wgs"] >= 1 and g["wg_waves"] in (4, 8) and (g["lds"] == 0 or g["wg_waves"] == 8 or form == "AND_TILED"), what
        if form == "AND_BAND_WALK":
            assert 2 <= g["bands"] <= 64 and 3 <= g["ch"] <= 16, what
    assert seen == set(FORMS), set(FORMS) - seen
