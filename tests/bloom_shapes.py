"""Database construction from sequences stated as data: the shared-set launch form of kmer_kernel (engine.hip
run_shared_kmer_pass: shared_lg != 0, lds_slots = 0, no work list, bloom_bits set -- one workgroup of KM_THREADS threads per
sequence whatever its length, ONE global distinct set for the whole sample, atomicOr into the filter) and the piece cut of
kwage_make_bloom (host.cpp) in front of it.  Host only: no device, no oracle.

- pieces(length, k): the piece cut -- pieces of PIECE = 2^16 start positions that overlap by k - 1 bases; the cut stops with
  the piece that reaches the sequence's end.  A sequence of no base has no piece.
- table_log2(total_pos): the shared set has 2^lg slots, the smallest lg >= MIN_SHARED_LOG2 with 2^lg >= 2 max(total_pos, 1),
  total_pos = the k-mer positions of all sequences (pieces) of the batch.
- CASES: what test_gpu_bloom_shapes.py runs.  A case: name, group, k, num_hash, L, the sequences (from a generator seeded by
  the name), the entry points -- "B": kwage_bloom_bits_from_batch + kwage_count_distinct_kmers on a Batch of the sequences as
  they are; "M": kwage_make_bloom into a file -- whether the sample is declared to hold no k-mer, and what the case is for.
  test_bloom_shapes_ledger.py checks on CPU that the two rules above are the sources', that every case of the piece cut
  has the pieces its name claims, that no filter is saturated, and that every named edge is present on both sides."""
import zlib
from collections import namedtuple

import numpy as np

PIECE = 1 << 16             # host.cpp kwage_make_bloom
MIN_SHARED_LOG2 = 10        # engine.hip run_shared_kmer_pass
WG = 256                    # kernels.hpp KM_THREADS: the shared-set form is always launched with it

_RC = str.maketrans("ACGTacgt", "TGCAtgca")
IUPAC = "RYSWKMBDHVN"       # letters of a sequence file that are no base


def pieces(length, k):
    """[(first, end)] of the pieces kwage_make_bloom cuts a sequence of `length` bases into."""
    out, s0 = [], 0
    while s0 < length:
        s1 = min(length, s0 + PIECE + (k - 1))
        out.append((s0, s1))
        if s1 == length:
            break
        s0 += PIECE
    return out


def cut(seqs, k):
    """The batch kwage_make_bloom hands to the device for these sequences."""
    return [s[a:b] for s in seqs for a, b in pieces(len(s), k)]


def positions(seq, k):
    return max(len(seq) - k + 1, 0)


def total_pos(seqs, k):
    return sum(positions(s, k) for s in seqs)


def table_log2(npos):
    lg = MIN_SHARED_LOG2
    while (1 << lg) < 2 * max(npos, 1):
        lg += 1
    return lg


def revcomp(s):
    return s.translate(_RC)[::-1]


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def put(s, off, ch):
    return s[:off] + ch + s[off + 1:]


Case = namedtuple("Case", "name group k num_hash L seqs entry empty why")
CASES = []


def add(name, group, k, nh, L, seqs, entry, why, empty=False):
    assert entry in ("B", "M", "BM") and all(c.name != name for c in CASES), name
    CASES.append(Case(name, group, k, nh, L, list(seqs), entry, empty, why))


def small_sample(rng):
    """60 random bases with an N in the middle, their reverse complement in lower case, and 200 random bases."""
    a = put(rand_seq(rng, 60), 30, "N")
    return [a, revcomp(a).lower(), rand_seq(rng, 200)]


# ---- 1. parameters ----------------------------------------------------------------------------------------------------------
PARAM_KS = (1, 2, 4, 15, 16, 27, 31, 32)
for _k in PARAM_KS:
    for _nh in (1, 5):
        _n = "params_k%d_h%d" % (_k, _nh)
        add(_n, 1, _k, _nh, 16, small_sample(_rng(_n)), "BM", "k-mer length %d (word mask, reverse complement) at %d hash(es)" % (_k, _nh))
for _nh in (1, 2, 3, 4, 5):
    _n = "params_k21_h%d" % _nh
    add(_n, 1, 21, _nh, 16, small_sample(_rng("params_k21")), "BM", "every hash count on one sample: hash h must not depend on num_hash")

# ---- 2. filter lengths --------------------------------------------------------------------------------------------------------
# ONE k-mer: the small sample saturates a short filter (at L = 4 it sets all 16 bits), and a saturated filter hides every error
ONE_KMER_LS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12)
for _L in ONE_KMER_LS:
    for _nh in (1, 2):
        _n = "len_L%d_h%d_one_kmer" % (_L, _nh)
        add(_n, 2, 31, _nh, _L, [rand_seq(_rng("len_one_kmer_h%d" % _nh), 31)], "BM",
            "2^%d bits%s: row_mask, and a filter of %d byte(s) in a dword of device memory" % (_L, " (less than a byte)" if _L < 3 else "", max(1, (1 << _L) // 8)))
add("len_L8_h1_sample", 2, 21, 1, 8, small_sample(_rng("len_sample")), "BM", "190 k-mers into 256 bits: many atomicOr into the same dwords")
add("len_L12_h5_sample", 2, 21, 5, 12, small_sample(_rng("len_sample")), "BM", "950 bits into 4096")
add("len_L32_h5_sample", 2, 21, 5, 32, small_sample(_rng("len_sample")), "BM",
    "L = 32 has its own row_mask branch (1u << 32 is not a mask); a 512 MiB filter, bit indices up to 2^32 - 1")

# ---- 3. lengths around k ------------------------------------------------------------------------------------------------------
AROUND_KS = (1, 31, 32)
for _k in AROUND_KS:
    _r = _rng("around_k%d" % _k)
    _lens = {"len_0": 0, "len_k_minus_1": _k - 1, "len_k": _k, "len_k_plus_1": _k + 1}
    for _what, _len in _lens.items():
        if _what == "len_k_minus_1" and _k == 1:
            continue                                    # (length 0 again)
        add("around_k%d_%s" % (_k, _what), 3, _k, 3, 16, [rand_seq(_r, _len)], "BM",
            "a sequence of %d base(s): %d k-mer(s)" % (_len, max(_len - _k + 1, 0)), empty=_len < _k)
    add("around_k%d_only_N" % _k, 3, _k, 3, 16, ["N" * (2 * _k + 5)], "BM", "no base at all", empty=True)
    _s = rand_seq(_r, 4 * _k + 3)
    add("around_k%d_N_every_k" % _k, 3, _k, 3, 16, ["".join("N" if i % _k == _k - 1 else c for i, c in enumerate(_s))], "BM",
        "runs of k - 1 bases: no valid k-mer", empty=True)
    _s = rand_seq(_r, 4 * (_k + 1) + 2)
    add("around_k%d_N_every_k_plus_1" % _k, 3, _k, 3, 16, ["".join("N" if i % (_k + 1) == _k else c for i, c in enumerate(_s))], "BM",
        "runs of exactly k bases: one valid k-mer between two N")
    add("around_k%d_iupac" % _k, 3, _k, 3, 16, ["".join(rand_seq(_r, _k + 2) + x for x in IUPAC + IUPAC.lower())], "BM",
        "every IUPAC letter that is no base, in both cases, ends a run of k + 2 bases")
    add("around_k%d_batch_without_kmer" % _k, 3, _k, 3, 16,
        ["", rand_seq(_r, _k - 1), "N" * 40, "".join("N" if i % _k == _k - 1 else c for i, c in enumerate(rand_seq(_r, 100))), "RYKM" * 10], "BM",
        "only sequences without a k-mer: a zero filter, distinct 0, the file still written", empty=True)
add("around_no_sequence", 3, 31, 3, 16, [], "BM",
    "a batch of no sequence: include/kwage_amd.h documents nothing for it; the code launches nothing and reports a zero filter and "
    "distinct 0, and kwage_make_bloom still writes the file -- asserted as found", empty=True)

# ---- 4. tile edges of the fixed 256-thread workgroup --------------------------------------------------------------------------
# One batch per (k, positions): the clean sequence first, then a sequence of its own for every offset of ONE invalid base from
# 255 - k to 256 + k - 1 -- in and just past the k - 1 characters that the first two tiles both stage.  Every variant is drawn
# on its own, so a k-mer lost in one of them is found in no other (k >= 31).  L = 20: up to 66 sequences of 512 k-mers would
# set most bits of a filter of 2^16.
TILE_KS = (1, 31, 32)
TILE_POSITIONS = (WG - 1, WG, WG + 1, 2 * WG, 2 * WG + 1)
for _k in TILE_KS:
    for _p in TILE_POSITIONS:
        _n = "tile_k%d_P%d" % (_k, _p)
        _r, _len = _rng(_n), _p + _k - 1
        _seqs = [rand_seq(_r, _len)]
        for _i, _off in enumerate(range(WG - 1 - _k, WG + _k)):
            if 0 <= _off < _len:
                _seqs.append(put(rand_seq(_r, _len), _off, "Nnx"[_i % 3]))
        add(_n, 4, _k, 2, 20, _seqs, "B", "%d positions: %d whole tile(s) of %d and %d left; one invalid base at every offset around the first tile edge"
            % (_p, _p // WG, WG, _p % WG))

# ---- 5. one set for the whole sample ------------------------------------------------------------------------------------------
_read = rand_seq(_rng("reads"), 150)
add("shared_4000_reads", 5, 31, 3, 16, [_read, revcomp(_read), _read.lower(), revcomp(_read).lower()] * 1000, "BM",
    "4000 workgroups insert the same 120 k-mers, in both strands and both cases of letters: counted once")
for _k in (31, 32):
    _base = rand_seq(_rng("overlap_k%d" % _k), 3 * _k + 40)
    _cutat = _k + 25
    add("shared_overlap_k%d_by_k_minus_1" % _k, 5, _k, 3, 16, [_base[:_cutat], _base[_cutat - (_k - 1):]], "BM", "two sequences overlapping by k - 1 bases: no shared k-mer")
    add("shared_overlap_k%d_by_k" % _k, 5, _k, 3, 16, [_base[:_cutat], _base[_cutat - _k:]], "BM", "two sequences overlapping by k bases: one shared k-mer")
add("shared_polyA_polyT_k32", 5, 32, 3, 16, ["A" * 40, "T" * 40, "A" * 32, "T" * 32], "BM",
    "word 0 against its all-ones reverse complement, the value of an empty slot (KM_EMPTY): one k-mer")
for _k in (2, 4, 16, 32):
    add("shared_palindromes_k%d" % _k, 5, _k, 3, 16, ["ACGT" * 16], "BM", "ACGT repeated at even k: words equal to their own reverse complement")
SLOT_STEP = 512             # 2 * 512 = 1024 slots = 2^MIN_SHARED_LOG2: the last total_pos of the smallest table
for _t in (SLOT_STEP - 1, SLOT_STEP, SLOT_STEP + 1):
    _r = _rng("slots_%d" % _t)
    add("shared_total_pos_%d" % _t, 5, 31, 3, 16, [rand_seq(_r, 200 + 30), rand_seq(_r, 300 + 30), rand_seq(_r, _t - 500 + 30)], "BM",
        "%d positions, all k-mers distinct: %d slots" % (_t, 1 << table_log2(_t)))

# ---- 6. the piece cut -----------------------------------------------------------------------------------------------------------
# 'A' throughout, with 200 random bases centred on every multiple of PIECE: the k-mers at a cut occur nowhere else (k >= 31),
# so a dropped one shows, and the expected set stays a few hundred words.
CUT_KS = (1, 2, 31, 32)
CUT_LENGTHS = {"P+k-2": lambda k: PIECE + k - 2, "P+k-1": lambda k: PIECE + k - 1, "P+k": lambda k: PIECE + k,
               "2P+k-1": lambda k: 2 * PIECE + k - 1, "2P+5": lambda k: 2 * PIECE + 5}


def cut_seq(rng, length):
    s = bytearray(b"A" * length)
    for m in range(0, length + 100, PIECE):
        a, b = max(m - 100, 0), min(m + 100, length)
        if a < b:
            s[a:b] = rand_seq(rng, b - a).encode()
    return s.decode()


def n_offsets(k):
    """The invalid base of a cut variant: the last start of the first piece, the first of the second, the last base the two share."""
    return sorted({PIECE - 1, PIECE, PIECE + k - 2})


for _k in CUT_KS:
    for _what, _fn in CUT_LENGTHS.items():
        _len = _fn(_k)
        _n = "cut_k%d_%s_pieces%d" % (_k, _what, len(pieces(_len, _k)))
        add(_n, 6, _k, 3, 16, [cut_seq(_rng(_n), _len)], "BM", "%d bases at k = %d: last piece of %d base(s)" % (_len, _k, pieces(_len, _k)[-1][1] - pieces(_len, _k)[-1][0]))
    for _what in ("P+k", "2P+5") if _k == 31 else ("2P+5",):
        _len = CUT_LENGTHS[_what](_k)
        for _off in n_offsets(_k):
            _n = "cut_k%d_%s_N_at_%d_pieces%d" % (_k, _what, _off, len(pieces(_len, _k)))
            add(_n, 6, _k, 3, 16, [put(cut_seq(_rng(_n), _len), _off, "N")], "BM", "an N at base %d, on the cut" % _off)
_r = _rng("cut_sample")
add("cut_k31_sample_pieces5", 6, 31, 3, 16, [cut_seq(_r, PIECE + 31), cut_seq(_r, 2 * PIECE + 5), rand_seq(_r, 40)], "BM",
    "two cut sequences, then a 40-base one: piece offsets behind a cut sequence")

BY_NAME = {c.name: c for c in CASES}


# ---- what a case must give, from the oracle handed in (computed once per case and kept) ------------------------------------------
_expected = {}


def distinct_seqs(seqs):
    """The sequences without exact repeats: the same k-mer set and filter (4000 reads are four strings)."""
    return list(dict.fromkeys(seqs))


def union_kmers(oracle, seqs, k):
    found = [oracle.unique_kmers(s, k) for s in distinct_seqs(seqs)]
    return np.unique(np.concatenate(found)) if found else np.zeros(0, dtype=np.uint64)


def expected(oracle, case):
    """(distinct canonical k-mers of the whole sample, sorted; the sorted distinct bit indices of its filter)."""
    if case.name not in _expected:
        km = union_kmers(oracle, case.seqs, case.k)
        idx = np.unique(oracle.row_indices(km, case.k, case.num_hash, case.L).astype(np.int64)) if len(km) else np.zeros(0, dtype=np.int64)
        _expected[case.name] = (km, idx)
    return _expected[case.name]
