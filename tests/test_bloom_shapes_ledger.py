"""The ledger of tests/bloom_shapes.py against the sources of database construction (no GPU): the piece constant and the
table rule the table restates are the ones host.cpp and engine.hip hold and the launch form is the one it describes, every
case of the piece cut has the pieces its name claims and the union of its pieces' k-mers is the whole sequence's, no
case's filter is saturated (a cap on the table, met with the oracle alone), and every named edge is present on both sides.
A constant edited in the sources without the table fails here, naming the constant."""
import os
import re

import numpy as np

from conftest import ROOT

import bloom_shapes as bs

CSRC = os.path.join(ROOT, "kwage_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: expected one match of %r in the sources, found %d" % (what, pattern, len(found))
    return found[0]


def group(g):
    return [c for c in bs.CASES if c.group == g]


def test_piece_cut_and_table_rule_are_the_sources():
    cpp, hip, hpp = source("host.cpp"), source("engine.hip"), source("kernels.hpp")
    make_bloom = cpp[cpp.index('extern "C" int kwage_make_bloom('):cpp.index("struct kwage_dbinfo")]
    lg = int(one(r"const uint64_t PIECE = 1u << (\d+);", make_bloom, "PIECE"))
    assert 1 << lg == bs.PIECE, "PIECE is 2^%d in host.cpp, %d in bloom_shapes.py" % (lg, bs.PIECE)
    # the cut: pieces of PIECE starts, overlap k - 1, stop with the piece that reaches the end
    one(r"for\(uint64_t s0 = b; s0 < e; s0 \+= PIECE\)\{\s*const uint64_t s1 = std::min\(e, s0 \+ PIECE \+ \(k - 1\)\);\s*"
        r"pieces\.append\(seqs \+ s0, s1 - s0\);\s*po\.push_back\(pieces\.size\(\)\);\s*if\(s1 == e\)\{ break; \}", make_bloom, "the piece loop of kwage_make_bloom")
    shared = hip[hip.index("int run_shared_kmer_pass("):hip.index('extern "C" int kwage_count_distinct_kmers(')]
    lg = int(one(r"uint32_t lg = (\d+);\s*while\(\(1ull << lg\) < 2\*std::max<uint64_t>\(L->total_pos, 1\)\)\{ \+\+lg; \}", shared, "MIN_SHARED_LOG2"))
    assert lg == bs.MIN_SHARED_LOG2, "the shared table starts at 2^%d slots in engine.hip, 2^%d in bloom_shapes.py" % (lg, bs.MIN_SHARED_LOG2)
    # the launch form the table describes: one workgroup of KM_THREADS per sequence, no LDS table, no work list, cleared set
    one(r"hipLaunchKernelGGL\(kmer_kernel, dim3\(b->n\), dim3\(KM_THREADS\), 0, ctx->stream, a\);", shared, "the launch of the shared-set form")
    one(r"a\.lds_slots = 0;", shared, "lds_slots")
    one(r"a\.chunk_q = nullptr; a\.chunk_t0 = nullptr;", shared, "the work list")
    one(r"a\.shared_lg = lg;", shared, "shared_lg")
    one(r"hipMemsetAsync\(sl->tables\.p, 0xFF, \(1ull << lg\)\*sizeof\(uint64_t\), ctx->stream\)", shared, "the table's memset")
    one(r"if\(a\.shared_lg\)\{\s*kmer_body<false, false>\(a, q, s0, len, 0, npos, a\.g_tables, a\.shared_lg,", hip, "kmer_kernel's shared-set branch")
    assert int(one(r"static constexpr int KM_THREADS = (\d+);", hpp, "KM_THREADS")) == bs.WG
    # the rules themselves, at values worked out by hand
    assert [bs.table_log2(p) for p in (0, 1, 511, 512, 513, 1024, 1025, 1 << 20)] == [10, 10, 10, 10, 11, 11, 12, 21]
    P = bs.PIECE
    assert bs.pieces(0, 31) == [] and bs.pieces(5, 31) == [(0, 5)]
    assert bs.pieces(P + 30, 31) == [(0, P + 30)] and bs.pieces(P + 31, 31) == [(0, P + 30), (P, P + 31)]
    assert bs.pieces(2 * P + 5, 31) == [(0, P + 30), (P, 2 * P + 5)] and bs.pieces(2 * P + 5, 1) == [(0, P), (P, 2 * P), (2 * P, 2 * P + 5)]
    assert bs.pieces(P, 1) == [(0, P)] and bs.pieces(P + 1, 1) == [(0, P), (P, P + 1)]


def test_every_cut_case_has_its_pieces_and_loses_no_kmer(oracle):
    cases = group(6)
    plain = {(c.k, len(c.seqs[0])) for c in cases if "_N_at_" not in c.name and len(c.seqs) == 1}
    assert plain == {(k, fn(k)) for k in bs.CUT_KS for fn in bs.CUT_LENGTHS.values()} and len(plain) == 20
    for k in bs.CUT_KS:
        got = {int(c.name.split("_N_at_")[1].split("_")[0]) for c in cases if c.k == k and "_N_at_" in c.name}
        assert got == set(bs.n_offsets(k)) and got >= {bs.PIECE - 1, bs.PIECE, bs.PIECE + k - 2}, (k, got)
    for c in cases:
        claimed = int(re.search(r"_pieces(\d+)$", c.name).group(1))
        cut = bs.cut(c.seqs, c.k)
        assert len(cut) == claimed == sum(len(bs.pieces(len(s), c.k)) for s in c.seqs), c.name
        assert all(len(p) <= bs.PIECE + c.k - 1 for p in cut), c.name
        whole = bs.expected(oracle, c)[0]
        assert np.array_equal(bs.union_kmers(oracle, cut, c.k), whole), c.name
        # the k-mer that straddles the first cut is in no other place: without the overlap it would be lost
        if c.k >= 31 and "_N_at_" not in c.name:
            s = c.seqs[0]
            straddle = oracle.unique_kmers(s[bs.PIECE - c.k + 1:bs.PIECE + c.k - 1], c.k)
            no_overlap = [s[a:a + bs.PIECE] for a in range(0, len(s), bs.PIECE)]
            lost = np.setdiff1d(straddle, bs.union_kmers(oracle, no_overlap, c.k))
            assert len(lost) == min(c.k - 1, len(s) - bs.PIECE), (c.name, len(lost))
    assert {(c.k, len(bs.cut(c.seqs, c.k))) for c in cases if len(c.seqs) == 1} == {(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (31, 1), (31, 2), (32, 1), (32, 2)}
    last = {(c.k, len(c.seqs[0]) - bs.pieces(len(c.seqs[0]), c.k)[-1][0]) for c in cases if len(c.seqs) == 1}
    assert {(k, k) for k in bs.CUT_KS} <= last, "a last piece of exactly one k-mer, at every k"


def test_no_filter_is_saturated(oracle):
    """A cap, not a measurement: a saturated filter hides every error, an empty one every loss."""
    for c in bs.CASES:
        km, idx = bs.expected(oracle, c)
        if c.empty:
            assert c.group == 3 and len(km) == 0 and len(idx) == 0, c.name
            continue
        assert len(km) > 0 and 0 < len(idx) <= len(km) * c.num_hash, c.name
        if c.L > 2:
            assert len(idx) < (1 << c.L), (c.name, "every bit of the filter is set")
    # why group 2 uses one k-mer: the small sample fills a 16-bit filter
    sample = bs.BY_NAME["len_L8_h1_sample"]
    assert len(np.unique(oracle.row_indices(bs.expected(oracle, sample)[0], sample.k, 1, 4))) == 16


def test_every_named_edge_is_present_on_both_sides(oracle):
    names = set(bs.BY_NAME)
    assert len(names) == len(bs.CASES) and all(c.why for c in bs.CASES)
    assert {c.group for c in bs.CASES} == {1, 2, 3, 4, 5, 6}
    assert all(c.entry == "B" for c in group(4)) and all(c.entry == "BM" for c in bs.CASES if c.group != 4)
    # 1: every k at one and five hashes, k = 21 at every hash count, all at L = 16 on the small sample
    assert {(c.k, c.num_hash) for c in group(1)} == {(k, h) for k in (1, 2, 4, 15, 16, 27, 31, 32) for h in (1, 5)} | {(21, h) for h in (1, 2, 3, 4, 5)}
    assert all(c.L == 16 and len(c.seqs) == 3 and c.seqs[0][30] == "N" and c.seqs[1].islower() and len(c.seqs[2]) == 200 for c in group(1))
    # 2: every short length with ONE k-mer at one and two hashes; 8 and 12 with the sample too; 32
    one_kmer = [c for c in group(2) if c.name.endswith("one_kmer")]
    assert {(c.L, c.num_hash) for c in one_kmer} == {(L, h) for L in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12) for h in (1, 2)}
    assert all(len(bs.expected(oracle, c)[0]) == 1 and len(c.seqs[0]) == c.k == 31 for c in one_kmer)
    assert {(c.L, c.num_hash) for c in group(2) if c.name.endswith("sample")} == {(8, 1), (12, 5), (32, 5)}
    # 3: around k at k = 1, 31, 32
    for k in bs.AROUND_KS:
        mine = {c.name[len("around_k%d_" % k):]: c for c in group(3) if c.name.startswith("around_k%d_" % k)}
        assert set(mine) == {"len_0", "len_k", "len_k_plus_1", "only_N", "N_every_k", "N_every_k_plus_1", "iupac", "batch_without_kmer"} | ({"len_k_minus_1"} if k > 1 else set())
        assert [len(mine[n].seqs[0]) for n in ("len_0", "len_k", "len_k_plus_1")] == [0, k, k + 1]
        assert len(bs.expected(oracle, mine["len_k"])[0]) == 1 and len(bs.expected(oracle, mine["len_k_plus_1"])[0]) in ((1, 2) if k == 1 else (2,))
        assert {n for n, c in mine.items() if c.empty} == {"len_0", "only_N", "N_every_k", "batch_without_kmer"} | ({"len_k_minus_1"} if k > 1 else set())
        assert len(mine["batch_without_kmer"].seqs) > 1 and bs.total_pos(mine["N_every_k"].seqs, k) > 0
        assert set(bs.IUPAC + bs.IUPAC.lower()) <= set(mine["iupac"].seqs[0]) and not set("ACGTacgt") & set(bs.IUPAC)
        # one valid k-mer between two N: runs of exactly k bases (the tail is shorter)
        runs = mine["N_every_k_plus_1"].seqs[0].split("N")
        assert all(len(run) <= k for run in runs) and sum(len(run) == k for run in runs) >= 4
    assert bs.BY_NAME["around_no_sequence"].seqs == [] and bs.BY_NAME["around_no_sequence"].empty
    # 4: both sides of the tile edges, an invalid base at every offset around the first one
    assert {(c.k, bs.positions(c.seqs[0], c.k)) for c in group(4)} == {(k, p) for k in (1, 31, 32) for p in (255, 256, 257, 512, 513)}
    for c in group(4):
        n = len(c.seqs[0])
        bad = sorted(next(i for i, ch in enumerate(s) if ch not in "ACGT") for s in c.seqs[1:])
        assert bad == [o for o in range(bs.WG - 1 - c.k, bs.WG + c.k) if 0 <= o < n], c.name
        assert all(len(s) == n and sum(ch not in "ACGT" for ch in s) == 1 for s in c.seqs[1:]), c.name
    # 5: one set
    reads = bs.BY_NAME["shared_4000_reads"]
    assert len(reads.seqs) == 4000 and len(bs.distinct_seqs(reads.seqs)) == 4 and len(bs.expected(oracle, reads)[0]) == 150 - 31 + 1
    assert any(s.islower() for s in reads.seqs) and bs.revcomp(reads.seqs[0]) == reads.seqs[1]
    for k in (31, 32):
        a, b = (bs.BY_NAME["shared_overlap_k%d_by_%s" % (k, w)] for w in ("k_minus_1", "k"))
        shared = [len(np.intersect1d(oracle.unique_kmers(c.seqs[0], k), oracle.unique_kmers(c.seqs[1], k))) for c in (a, b)]
        assert shared == [0, 1], (k, shared)
    poly = bs.BY_NAME["shared_polyA_polyT_k32"]
    assert poly.k == 32 and bs.expected(oracle, poly)[0].tolist() == [0]
    for k in (2, 4, 16, 32):
        c = bs.BY_NAME["shared_palindromes_k%d" % k]
        words, _ = oracle.canonical_kmers(c.seqs[0], k)
        assert c.seqs == ["ACGT" * 16] and len(words) == 64 - k + 1 and any(bs.revcomp(c.seqs[0][i:i + k]) == c.seqs[0][i:i + k] for i in range(4))
        assert len(bs.expected(oracle, c)[0]) == 3                # ACGT.., CGTA.. = TACG.. reversed, GTAC..: two of them their own reverse complement
    slots = {}
    for t in (511, 512, 513):
        c = bs.BY_NAME["shared_total_pos_%d" % t]
        assert bs.total_pos(c.seqs, c.k) == t == len(bs.expected(oracle, c)[0]), c.name          # all k-mers distinct
        slots[t] = 1 << bs.table_log2(t)
    assert slots == {511: 1024, 512: 1024, 513: 2048} and bs.SLOT_STEP == 512
    # 6: (its own test above) the sample of several sequences puts a short one behind two cut ones
    c = bs.BY_NAME["cut_k31_sample_pieces5"]
    assert [len(bs.pieces(len(s), 31)) for s in c.seqs] == [2, 2, 1] and len(c.seqs[2]) == 40
