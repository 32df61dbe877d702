"""The device ordering of long hit lists (kwage_amd/csrc/hit_sort.hip) against a plain reference, on an MI355X.

Directly: order_hits_by_runs is fed the run tables and raw lists of tests/hit_order_cases.py by a stand-alone driver
(tests/device/hit_order_driver.hip, built from hit_sort.hip itself), and what it leaves in its scratch block is compared
byte for byte with the numpy reference -- the scan over more than 1024 blocks of the table, runs from 1 to 65535
records, blocks of empty entries, tails of every loop, and a table that accounts for fewer records than the list holds.

Through the search: a run table of more than 2^20 entries, and irregular run lengths from every kernel form that
reserves hit slots."""
import os
import subprocess

import numpy as np
import pytest

import hit_order_cases as hc
from ordered_list_forms import NARROW_MIN_QUERIES, drive_every_kernel_form, queries_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ka():
    import kwage_amd
    return kwage_amd


@pytest.fixture(scope="module")
def ctx(ka):
    c = ka.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------
# order_hits_by_runs itself
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driven(tmp_path_factory):
    """Every case through one run of the driver (a child process; its first error ends it): {name: path of its output}."""
    d = tmp_path_factory.mktemp("hit_order")
    exe = hc.build_driver(d)
    paths = []
    for name in hc.names():
        c = hc.case(name)
        p = os.path.join(str(d), name + ".case")
        with open(p, "wb") as f:
            f.write(np.array([c.table.size, c.n_hits], dtype="<u8").tobytes())
            f.write(c.table.astype("<u8").tobytes())
            f.write(hc.raw_list(c.n_hits).astype("<u4").tobytes())
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return {name: p + ".out" for name, p in zip(hc.names(), paths)}


@pytest.mark.parametrize("name", hc.names())
def test_order_hits_by_runs_against_the_reference(driven, name):
    c = hc.case(name)
    out = np.fromfile(driven[name], dtype=np.uint8)
    assert out.size == 16 + c.n_hits * 4 * hc.HIT_WORDS
    total, guards = (int(x) for x in out[:16].view("<u8"))
    want_total, want = hc.reference(c.table, hc.raw_list(c.n_hits))
    assert want_total == int(hc.lens_of(c.table).sum())
    if c.edge == "under_claim":
        assert want_total == c.n_hits - hc.UNDER_CLAIM
    else:
        assert want_total == c.n_hits
    assert total == want_total, "the word at *d_total is the table's record total"
    # the ordered records byte for byte; behind the table's total nothing is written
    want_bytes = np.concatenate([want.astype("<u4").view(np.uint8).reshape(-1),
                                 np.full((c.n_hits - want_total) * 4 * hc.HIT_WORDS, hc.SENTINEL, dtype=np.uint8)])
    got = out[16:]
    if not np.array_equal(got, want_bytes):
        bad = np.flatnonzero(np.any(got.reshape(-1, 12) != want_bytes.reshape(-1, 12), axis=1))
        raise AssertionError("%d of %d records differ, the first at %d: got %s, want %s" % (
            bad.size, c.n_hits, bad[0], got.reshape(-1, 12)[bad[0]].view("<u4"), want_bytes.reshape(-1, 12)[bad[0]].view("<u4")))
    assert guards == 3, "bytes outside the scratch block of hit_order_scratch_bytes() were written (bit 0: below, bit 1: above)"


# ---------------------------------------------------------------------------------------------
# the same edges through the search
# ---------------------------------------------------------------------------------------------
def test_run_table_beyond_2_pow_20_entries(ka, ctx):
    """180 000 short reads against three columns: the run table has queries x runs_per_query entries, more than the
    2^20 that 1024 scan threads take one block each of, so run_scan_sums sums and rewrites stretches of block sums.  At a
    threshold that truncates to 0 every column matches every query with a k-mer: the list is known in closed form."""
    n_cols, n_queries = 3, 180000
    g = ka.Group(ctx, 31, 1, 6, n_cols)
    g.add_random_columns(n_cols, 11, 128)
    g.finalize()
    # engine.hip, search_submit: entries per query of the run table
    kib = -(-(g.row_stride // 16) // 64)
    walk_tile = min(max(ctx.get_tuning("walk_tile_kib"), 1), 16)
    runs_per_query = kib + -(-kib // walk_tile) + 4
    assert n_queries * runs_per_query > 1 << 20, (g.row_stride, walk_tile, runs_per_query)
    assert -(-n_queries * runs_per_query // hc.ENTRIES_PER_BLOCK) > hc.SCAN_THREADS

    rng = np.random.default_rng(180000)
    lens = rng.integers(31, 61, size=n_queries)
    lens[np.arange(n_queries) % 7 == 3] = 4          # some without a k-mer
    ends = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(ends[-1]))].tobytes()
    seqs = [bases[e - n:e] for e, n in zip(ends.tolist(), lens.tolist())]
    b = ka.Batch(ctx, seqs)
    live = np.flatnonzero(lens >= 31).astype(np.uint32)
    assert 0 < n_queries - len(live) and len(live) * n_cols > 8192

    def check(r):
        assert np.array_equal(np.flatnonzero(r.num_query_kmer > 0), live)
        assert len(r.hits) == len(live) * n_cols
        assert np.array_equal(r.hits["query"], np.repeat(live, n_cols)), r.search_kernel
        assert np.array_equal(r.hits["column"], np.tile(np.arange(n_cols, dtype=np.uint32), len(live))), r.search_kernel

    r = g.search(b, 0.0001)
    check(r)
    with ctx.tuning(narrow=0):
        wide = g.search(b, 0.0001)
    assert "narrow" not in wide.search_kernel, wide.search_kernel
    check(wide)
    with ctx.tuning(hit_sort_host=1):
        by_host = g.search(b, 0.0001)
    assert np.array_equal(by_host.hits, r.hits) and np.array_equal(by_host.hits, wide.hits)
    b.close()
    g.close()


def irregular_columns(pattern, n_cols):
    rng = np.random.default_rng(7 * n_cols + len(pattern))      # fixed: the same columns in every run
    if pattern == "one-in-100":
        return rng.random(n_cols) < 1 / 100
    assert pattern == "one-in-2000-and-a-stretch"
    ones = rng.random(n_cols) < 1 / 2000
    first_byte = (n_cols // 3 // 8) | 1                          # an odd byte offset
    ones[8 * first_byte:8 * first_byte + min(n_cols // 4, 9000)] = True
    return ones


@pytest.mark.parametrize("n_cols", [4000, 40000, 300000])
@pytest.mark.parametrize("pattern", ["one-in-100", "one-in-2000-and-a-stretch"])
def test_irregular_runs_come_back_ordered_from_every_kernel_form(ka, ctx, pattern, n_cols):
    """test_gpu_parity.py's test_long_lists_come_back_ordered_from_every_kernel_form with columns that make the runs
    irregular: scattered all-ones columns (most 64-column steps report nothing or one record), or the same thinner plus one
    solid stretch that begins inside a byte-odd step (full runs beside empty ones).  Same knobs, same kernel names.

    Which form runs is decided by the row width and the batch size, never by the columns' contents, so both patterns
    reach the forms their width reaches: the narrow kernels only at 4000 columns (rows of at most 32 units of 16 bytes,
    batches of 64 queries or more), the early-exit screen from 64 units on (not at 4000), the walk form from 128 units on
    (not at 4000), band after band up to 1024 units (not at 300 000)."""
    ones = irregular_columns(pattern, n_cols)
    n_ones = int(ones.sum())
    assert 0 < n_ones < n_cols // 3
    # (run lengths differ: steps of 64 columns with no, one and several all-ones columns)
    per_step = np.add.reduceat(ones, np.arange(0, n_cols, 64))
    assert np.count_nonzero(per_step == 0) > len(per_step) // 8 and len(set(per_step.tolist())) >= 3
    # (rows narrow enough for the narrow kernels get the batch size those kernels ask for, or the knob alone would not reach them)
    n_queries = queries_for(n_ones, at_least=NARROW_MIN_QUERIES if n_cols <= 4096 else (36 if n_cols <= 40000 else 24))
    seen = set(drive_every_kernel_form(ka, ctx, n_cols, ones, n_queries, seed=n_cols + 1))
    assert {"and_kernel<1,", "and_kernel<2,", "and_kernel<4,", "and_kernel<", "count_kernel<", "count_walk_kernel<"} <= seen
    assert ("and_narrow_kernel<" in seen) == ("count_narrow_kernel<" in seen) == (n_cols == 4000)
    assert ("and_screen_kernel<" in seen) == ("count_screen_kernel<" in seen) == ("and_walk_kernel<" in seen) == (n_cols > 4000)
    assert ("and_band_walk_kernel<" in seen) == (n_cols == 40000)
