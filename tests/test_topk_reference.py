"""CPU: the top-k tests' reference (topk_reference.py) pinned to a brute-force statement of the contract -- the addressed
rows unpacked, ANDed across the hash functions, summed in int64, the floor (unsigned)(float32(t) * n), the eligible real
columns sorted by (count descending, column ascending) and cut at k."""
import numpy as np
import pytest

import topk_reference as ref


def _brute(img, nf, kmers, kmer, num_hash, L, oracle):
    rows = oracle.row_indices(kmers, kmer, num_hash, L)                        # [n, num_hash]
    bits = np.unpackbits(img, axis=1, bitorder="little")[:, :nf].astype(bool)
    match = np.logical_and.reduce(bits[rows], axis=1) if len(kmers) else np.zeros((0, nf), bool)
    return match.sum(axis=0, dtype=np.int64)


def _brute_select(counts, valid, t, n, k):
    if n == 0:
        return []
    f = int(np.float32(t) * np.float32(n))
    elig = [(int(c), int(counts[c])) for c in valid if counts[c] >= f]
    elig.sort(key=lambda cm: (-cm[1], cm[0]))
    return sorted(elig[:k])


@pytest.mark.parametrize("num_hash", [1, 2, 3, 4, 5])
def test_reference_matches_brute_force(oracle, num_hash):
    rng = np.random.default_rng(500 + num_hash)
    kmer, L = 15, 7
    files_nf = [37, 200, 5]
    genome = ref.rand_seq(rng, 400)
    files, span, images = [], 0, []
    for f, nf in enumerate(files_nf):
        bits = rng.random((1 << L, nf)) < (0.85 if num_hash > 2 else 0.5)
        for c in (0, nf // 2, nf - 1):                                           # planted ties: equal columns ...
            bits[:, c] = bits[:, 0]
        if nf > 10:                                                              # ... and columns holding every row
            for c in (3, 9):
                bits[oracle.row_indices(oracle.unique_kmers(genome, kmer), kmer, num_hash, L).reshape(-1), c] = True
        img = ref.pack_columns(bits, rng)
        files.append((span, img, nf, None))
        images.append((span, img, nf))
        span += ((nf + 127) // 128) * 128
    # one file as copies of a base block (the wide groups' construction): column j is base column cmap[j]
    cmap = (np.arange(150) * 7 + 3) % files_nf[1]
    bits = np.unpackbits(images[1][1], axis=1, bitorder="little")[:, :files_nf[1]].astype(bool)[:, cmap]
    copy_img = ref.pack_columns(bits, rng)
    files.append((span, images[1][1], 150, cmap))
    images.append((span, copy_img, 150))
    span += 256
    queries = [genome, genome[50:120], ref.rand_seq(rng, 60), genome[:30] + ref.rand_seq(rng, 30), "ACGTACG"]
    for q in queries:
        kmers = oracle.unique_kmers(q, kmer)
        n = len(kmers)
        brute = np.full(span, -1, dtype=np.int64)
        for first, img, nf in images:
            brute[first:first + nf] = _brute(img, nf, kmers, kmer, num_hash, L, oracle)
        counts = ref.column_counts(oracle, files, span, kmer, num_hash, L, kmers)
        assert np.array_equal(counts, brute), q
        valid = np.flatnonzero(brute >= 0)
        if q is genome:
            assert (brute[[3, 9]] == n).all()
        for t in (0.0, 0.3, 0.5, 0.77, 1.0):
            f = oracle.query_threshold(float(np.float32(t)), n)
            assert f == int(np.float32(t) * np.float32(n)), (t, n)
            for k in (1, 2, 3, 5, 40, 64, 65, 300, 1024):
                exp = _brute_select(brute, valid, t, n, k)
                got, _ = ref.expected_hits(oracle, [(n, counts)], t, k)
                assert [(int(c), int(m)) for _, c, m in got.tolist()] == exp, (num_hash, t, k)


def test_cut_threshold_hits_is_the_same_rule():
    rng = np.random.default_rng(3)
    recs = []
    for q in range(7):
        cols = np.sort(rng.choice(5000, size=rng.integers(0, 900), replace=False))
        for c in cols:
            recs.append((q, c, int(rng.integers(0, 6))))          # many ties
    hits = np.array(recs, dtype=ref.HIT_DTYPE)
    for k in (1, 5, 64, 1024):
        got = ref.cut_threshold_hits(hits, k)
        exp = []
        for q in range(7):
            mine = [(int(c), int(m)) for qq, c, m in recs if qq == q]
            mine.sort(key=lambda cm: (-cm[1], cm[0]))
            exp += [(q, c, m) for c, m in sorted(mine[:k])]
        assert got.tolist() == exp, k
