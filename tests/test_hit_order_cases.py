"""The cases of tests/hit_order_cases.py against the edges of kwage_amd/csrc/hit_sort.hip they are there for (no GPU):
every case's property is recomputed here from its table, so a case that stops covering its edge fails, naming it; the
vectorised reference is checked against a loop over the runs; and the stand-alone driver that feeds the cases to the
device code (tests/device/hit_order_driver.hip) cross-compiles for gfx950."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import ROOT

import hit_order_cases as hc

CSRC = hc.CSRC


@pytest.mark.skipif(not (os.path.exists(hc.HIPCC) or shutil.which(hc.HIPCC)), reason="hipcc not found")
def test_driver_cross_compiles(tmp_path):
    exe = hc.build_driver(tmp_path)
    assert os.path.getsize(exe) > 0 and os.access(exe, os.X_OK)


def test_constants_restate_hit_sort_hip():
    src = open(os.path.join(CSRC, "hit_sort.hip")).read()

    def const(name):
        return re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src).group(1).strip()
    assert const("ORDER_THREADS") == "256" and const("ENTRIES_PER_THREAD") == str(hc.ENTRIES_PER_THREAD)
    assert const("ENTRIES_PER_BLOCK") == "ORDER_THREADS*ENTRIES_PER_THREAD" and hc.ENTRIES_PER_BLOCK == 256 * hc.ENTRIES_PER_THREAD
    assert const("SCAN_THREADS") == str(hc.SCAN_THREADS) and const("COPY_CHUNK") == str(hc.COPY_CHUNK)
    drv = open(os.path.join(ROOT, "tests", "device", "hit_order_driver.hip")).read()
    assert int(re.search(r"SENTINEL\s*=\s*(0x[0-9A-Fa-f]+);", drv).group(1), 16) == hc.SENTINEL
    assert int(re.search(r"GUARD_BYTES\s*=\s*(\d+);", drv).group(1)) >= 4096


def block_records(lens):
    pad = -lens.size % hc.ENTRIES_PER_BLOCK
    return np.concatenate([lens, np.zeros(pad, np.int64)]).reshape(-1, hc.ENTRIES_PER_BLOCK).sum(axis=1)


@pytest.mark.parametrize("name", hc.names())
def test_every_case_is_a_table_the_engine_could_write(name):
    c = hc.case(name)
    lens, first = hc.lens_of(c.table), hc.firsts_of(c.table)
    total = int(lens.sum())
    assert c.table.dtype == np.uint64 and c.table.ndim == 1 and c.table.size >= 1
    assert 1 <= total <= c.n_hits, "a table never claims more records than the list holds, and no list is empty"
    assert np.all(c.table[lens == 0] == 0)
    # the runs pack the raw list: disjoint, no gap (an under-claiming table leaves exactly the records it gave up)
    nz = np.flatnonzero(lens)
    order = nz[np.argsort(first[nz])]
    gaps = np.diff(np.concatenate([first[order], [c.n_hits]])) - lens[order]
    assert first[order][0] == 0 and gaps.min() >= 0 and gaps.sum() == c.n_hits - total
    if nz.size > 8:
        assert not np.array_equal(order, nz), "the runs lie in the raw list in key order: nothing to put in order"
    raw = hc.raw_list(c.n_hits)
    assert len(np.unique(raw, axis=0)) == c.n_hits and len(np.unique(raw[:, 1])) > c.n_hits * 0.99
    assert not np.any(np.all(raw.view(np.uint8) == hc.SENTINEL, axis=1)), "a record must not look like untouched scratch"


@pytest.mark.parametrize("name", hc.names())
def test_every_case_covers_its_edge(name):
    c = hc.case(name)
    lens = hc.lens_of(c.table)
    n_runs, total = lens.size, int(lens.sum())
    to = np.cumsum(lens) - lens
    nz = np.flatnonzero(lens)
    nblocks = -(-n_runs // hc.ENTRIES_PER_BLOCK)
    per_block = block_records(lens)
    assert per_block.size == nblocks
    if c.edge == "n_runs":
        assert n_runs == c.want[0] and lens[-1] > 0
    elif c.edge == "scan":
        want_blocks, want_per = c.want
        per = -(-nblocks // hc.SCAN_THREADS)
        assert (nblocks, per) == (want_blocks, want_per) and n_runs % hc.ENTRIES_PER_BLOCK != 0
        idle = sum(1 for t in range(hc.SCAN_THREADS) if min(nblocks, t * per) == nblocks)      # lo == hi == nblocks
        assert (idle >= 1) == (nblocks > hc.SCAN_THREADS) and (nblocks != 1025 or idle >= 1)
        assert 0.005 < nz.size / n_runs < 0.02 and 100000 <= c.n_hits < 500000
        assert per_block[-1] > 0 and np.count_nonzero(per_block) > nblocks * 0.99
    elif c.edge == "first_block_empty":
        assert nblocks > 2 and per_block[0] == 0 and np.all(per_block[1:] > 0)
    elif c.edge == "last_block_empty":
        assert nblocks > 2 and per_block[-1] == 0 and np.all(per_block[:-1] > 0)
    elif c.edge == "alternate_blocks_empty":
        assert nblocks >= 8 and np.all(per_block[1::2] == 0) and np.all(per_block[0::2] > 0)
    elif c.edge == "late_start":
        assert nz[0] > 4096 and nz[0] % hc.ENTRIES_PER_BLOCK != 0
    elif c.edge == "last_entry":
        assert lens[-1] > 0 and n_runs % hc.ENTRIES_PER_THREAD == 1
    elif c.edge == "all_ones":
        assert set(lens.tolist()) == {0, 1} and c.n_hits >= 3 * hc.COPY_CHUNK + 1
        starts = np.bincount(to[nz] // hc.COPY_CHUNK)
        assert np.all(starts[:3] == hc.COPY_CHUNK), "2048 runs start in a chunk of 2048 records"
    elif c.edge == "longest":
        k = int(np.argmax(lens))
        assert lens[k] == hc.MAX_RUN == 65535 and to[k] % hc.COPY_CHUNK not in (0, hc.COPY_CHUNK - 1)
        assert (to[k] + lens[k] - 1) // hc.COPY_CHUNK - to[k] // hc.COPY_CHUNK >= 31
        assert k > 0 and np.all(lens[:k] == 1) and k + 1 < n_runs and np.all(lens[k + 1:] == 1)
    elif c.edge == "kernel_lengths":
        have = set(lens.tolist())
        assert {0, 8192, 32768} <= have and have <= set(range(65)) | {8192, 32768} and len(have & set(range(1, 65))) >= 60
        assert np.count_nonzero(lens == 8192) >= 4 and np.count_nonzero(lens == 32768) >= 2 and np.count_nonzero(lens == 0) > n_runs // 4
    elif c.edge == "n_hits":
        assert c.n_hits == total == c.want[0]
    elif c.edge == "under_claim":
        assert total == c.want[0] == c.n_hits - hc.UNDER_CLAIM and lens[nz[-1]] >= 1
    else:
        raise AssertionError("no check for edge %r" % c.edge)


def test_the_case_list_holds_what_it_must():
    by_edge = {}
    for n in hc.names():
        by_edge.setdefault(hc.case(n).edge, []).append(hc.case(n))
    assert sorted(c.want[0] for c in by_edge["n_runs"]) == [1, 3, 4, 5, 1023, 1024, 1025]
    assert sorted(c.want for c in by_edge["scan"]) == [(1024, 1), (1025, 2), (2049, 3)]
    assert {1, 2047, 2048, 2049} <= {c.want[0] for c in by_edge["n_hits"]}
    assert {"first_block_empty", "last_block_empty", "alternate_blocks_empty", "late_start", "last_entry", "all_ones", "longest",
            "kernel_lengths", "under_claim"} <= set(by_edge)
    # one under-claiming table ends in an earlier chunk of run_copy than its list does
    assert any(c.want[0] // hc.COPY_CHUNK < (c.n_hits - 1) // hc.COPY_CHUNK for c in by_edge["under_claim"])


def test_reference_agrees_with_a_loop_over_the_runs():
    small = [n for n in hc.names() if hc.case(n).n_hits <= hc.SMALL]
    assert len(small) >= 12 and {"under_claim", "n_runs", "n_hits", "all_ones"} <= {hc.case(n).edge for n in small}
    for n in small:
        c = hc.case(n)
        raw = hc.raw_list(c.n_hits)
        total, ordered = hc.reference(c.table, raw)
        total2, ordered2 = hc.reference_loop(c.table, raw)
        assert total == total2 and ordered.dtype == ordered2.dtype and np.array_equal(ordered, ordered2), n


def test_reference_on_a_table_written_out_by_hand():
    # runs in key order: 2 records at slot 3, none, 3 records at slot 0, 1 record at slot 5
    table = np.array([3 << 16 | 2, 0, 0 << 16 | 3, 5 << 16 | 1], dtype=np.uint64)
    raw = hc.raw_list(6)
    total, ordered = hc.reference(table, raw)
    assert total == 6 and ordered[:, 0].tolist() == [3, 4, 0, 1, 2, 5]
