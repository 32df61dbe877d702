"""The ledger of tests/kmer_shapes.py against the sources of the k-mer stage (no GPU): the dispatch constants the table
restates are the ones kernels.hpp and engine.hip hold, every batch of the table lists the form those rules give it, and
the batches together reach every workgroup size, every LDS table size and both sides of every edge between two forms.
A constant edited in the sources without the table fails here, naming the constant."""
import os
import re

from conftest import ROOT

import kmer_shapes as ks

CSRC = os.path.join(ROOT, "kwage_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: expected one match of %r in the sources, found %d" % (what, pattern, len(found))
    return found[0]


def test_dispatch_constants_are_the_sources():
    hpp, hip = source("kernels.hpp"), source("engine.hip")
    for name in ("KM_THREADS", "KM_LDS_SLOTS", "KM_CHUNK"):
        value = int(one(r"static constexpr \w+ %s = (\d+);" % name, hpp, name))
        assert value == getattr(ks, name), "%s is %d in kernels.hpp, %d in kmer_shapes.py" % (name, value, getattr(ks, name))
    small, mid = one(r"threads = \(L->max_pos <= (\d+)\) \? 64 : \(L->max_pos <= (\d+)\) \? 128 : KM_THREADS;", hip,
                     "the workgroup-size line of launch_kmer_kernels")
    assert int(small) == ks.WG64_MAX_POS, "64-thread threshold is %s in engine.hip, WG64_MAX_POS = %d in kmer_shapes.py" % (small, ks.WG64_MAX_POS)
    assert int(mid) == ks.WG128_MAX_POS, "128-thread threshold is %s in engine.hip, WG128_MAX_POS = %d in kmer_shapes.py" % (mid, ks.WG128_MAX_POS)
    # the table-size rule: the launch's table and both copies of table_log2 start at 64 slots and double up to 2 * positions
    slots = int(one(r"uint32_t slots = (\d+);\s*while\(slots < KM_LDS_SLOTS && slots < 2\*L->max_pos\)\{ slots \*= 2; \}", hip, "MIN_SLOTS"))
    assert slots == ks.MIN_SLOTS == 1 << ks.MIN_TABLE_LOG2, "MIN_SLOTS: %d in engine.hip, %d in kmer_shapes.py" % (slots, ks.MIN_SLOTS)
    for text, fn in ((hpp, "table_log2"), (hip, "host_table_log2")):
        lg = int(one(r"uint32_t %s\(uint64_t npos\)\s*\{[^}]*?uint32_t lg = (\d+);\s*while\(\(1ull << lg\) < 2\*npos\)\{ \+\+lg; \}" % fn, text, fn))
        assert lg == ks.MIN_TABLE_LOG2, "MIN_TABLE_LOG2: %s starts at %d, kmer_shapes.py at %d" % (fn, lg, ks.MIN_TABLE_LOG2)
    # the per-query choice of kmer_kernel and the host's cut of the work list: the same three tests
    one(r"if\(\(1ull << lg\) <= a\.lds_slots\)\{\s*kmer_body<true, false>", hip, "kmer_kernel's LDS branch")
    one(r"else if\(npos <= KM_CHUNK\)\{\s*kmer_body<false, false>", hip, "kmer_kernel's unreachable branch")
    one(r"is_long = npos && \(1ull << host_table_log2\(npos\)\) > KM_LDS_SLOTS;", hip, "batch_prepare's is_long")
    one(r"if\(!is_long \|\| npos <= KM_CHUNK\)\{ chunk_q\.push_back\(i\); chunk_t0\.push_back\(0\); continue; \}", hip, "batch_prepare's single chunk")
    one(r"for\(uint64_t t0 = 0; t0 < npos; t0 \+= KM_CHUNK\)\{ chunk_q\.push_back\(i\);", hip, "batch_prepare's chunk loop")
    assert ks.WORKGROUP_SIZES == (64, 128, ks.KM_THREADS) and ks.KM_CHUNK % ks.KM_THREADS == 0
    assert ks.MULTI_EDGE == ks.KM_LDS_SLOTS // 2 and ks.THREAD_EDGES == (ks.WG64_MAX_POS, ks.WG128_MAX_POS)
    assert ks.SLOT_EDGES == tuple(s // 2 for s in (64, 128, 256, 512, 1024, 2048)) and 2 * ks.SLOT_EDGES[-1] < ks.KM_LDS_SLOTS


def test_every_batch_lists_the_form_the_rules_give():
    assert ks.MAX_POS == [1, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048, 2049, 3072,
                          3073, 4097, 5000]
    for b in ks.BATCHES:
        assert b.form == ks.form(b.max_pos), (b, ks.form(b.max_pos))
        assert b.form.finish == (b.form.chunks > 1) == (b.max_pos > ks.MULTI_EDGE), b
    # the rules themselves, at values worked out by hand
    assert [ks.threads(p) for p in (1, 192, 193, 768, 769, 10 ** 6)] == [64, 64, 128, 128, 256, 256]
    assert [ks.lds_slots(p) for p in (0, 1, 32, 33, 1024, 1025, 2048, 2049, 10 ** 6)] == [64, 64, 64, 128, 2048, 4096, 4096, 4096, 4096]
    assert [ks.table_log2(p) for p in (1, 32, 33, 2048, 2049, 4096, 4097)] == [6, 6, 7, 12, 13, 13, 14]
    assert [ks.chunks(p, 4096) for p in (2048, 2049, 3072, 3073, 4096, 4097, 5000)] == [1, 3, 3, 4, 4, 5, 5]


def test_unreachable_branch_is_unreachable():
    """A query takes a global set only with more than KM_CHUNK positions, whatever the batch's longest query is."""
    assert len(ks.UNREACHABLE) == 1 and all("P > 2048" in why for why in ks.UNREACHABLE.values())
    for max_pos in list(range(1, 2 * ks.KM_LDS_SLOTS + 2)) + [10 ** 5, 2 ** 24]:
        slots = ks.lds_slots(max_pos)
        for npos in {1, max_pos // 2, max_pos - 1, max_pos, ks.KM_CHUNK, ks.KM_CHUNK + 1, ks.MULTI_EDGE, ks.MULTI_EDGE + 1}:
            if 0 < npos <= max_pos and not ks.in_lds(npos, slots):
                assert npos > ks.MULTI_EDGE > ks.KM_CHUNK and ks.chunks(npos, slots) >= 3, (max_pos, npos)


def test_batches_reach_every_form_and_both_sides_of_every_edge():
    forms = [b.form for b in ks.BATCHES]
    assert {f.threads for f in forms} == set(ks.WORKGROUP_SIZES)
    sizes, s = [], ks.MIN_SLOTS
    while s <= ks.KM_LDS_SLOTS:
        sizes.append(s)
        s *= 2
    assert {f.slots for f in forms} == set(sizes), sorted({f.slots for f in forms})
    have = set(ks.MAX_POS)
    for edge in ks.THREAD_EDGES + ks.SLOT_EDGES + (ks.MULTI_EDGE,):
        assert edge in have and edge + 1 in have, "edge %d / %d lacks a side" % (edge, edge + 1)
    for edge, fn in [(e, ks.threads) for e in ks.THREAD_EDGES] + [(e, ks.lds_slots) for e in ks.SLOT_EDGES]:
        assert fn(edge) != fn(edge + 1), edge                    # (they are edges)
    assert not ks.form(ks.MULTI_EDGE).finish and ks.form(ks.MULTI_EDGE + 1).finish
    # every form change between 1 and the largest batch is one of those edges
    changes = [p for p in range(1, max(have)) if ks.form(p)[:2] + (ks.form(p).finish,) != ks.form(p + 1)[:2] + (ks.form(p + 1).finish,)]
    assert set(changes) == set(ks.THREAD_EDGES + ks.SLOT_EDGES + (ks.MULTI_EDGE,)), changes
    multi = [p for p in have if p > ks.MULTI_EDGE]
    one_left = {p for p in multi if p % ks.KM_CHUNK == 1}
    assert {ks.chunks(p, ks.KM_LDS_SLOTS) for p in one_left} >= {3, 4, 5}, "a last chunk of exactly one position, at 3, 4 and 5 chunks"
    assert any(p % ks.KM_CHUNK == 0 for p in multi), "a query of whole chunks"
    assert any(p % ks.KM_CHUNK and (p % ks.KM_CHUNK) % ks.KM_THREADS > 1 for p in multi), "a last chunk that ends inside a tile"
