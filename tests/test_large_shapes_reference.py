"""tests/large_shapes.py against the CPU oracle on a group small enough to hold whole: what the helpers make of the
addressed rows alone must be what oracle.search_image makes of the full image."""
import numpy as np
import pytest

import large_shapes as ls
from topk_reference import ORACLE_ALL, pack_columns, rand_bits

K, NH, L, W = 21, 3, 10, 300


@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(610)
    genome = ls.random_dna(rng, 700)
    bits = rand_bits(rng, (1 << L, W), 0.5)
    real = np.ones(W + 4, dtype=bool)
    real[[17, 128, 299]] = False                         # pad columns that hold garbage
    real[W:] = False
    filters = np.stack([oracle.bloom_bits_from_sequences([genome], K, NH, L), np.full((1 << L) // 8, 255, dtype=np.uint8),
                        np.zeros((1 << L) // 8, dtype=np.uint8), rng.integers(0, 256, size=(1 << L) // 8, dtype=np.uint8)])
    known = [5, 64, 65, 290]
    for c, f in zip(known, filters):
        bits[:, c] = np.unpackbits(f, bitorder="little").astype(bool)
    image = pack_columns(bits, rng, pad_bytes=1)         # garbage behind column W too
    queries = [genome[40:190], ls.mutated(genome[300:520], 37), ls.random_dna(rng, 90), "", genome[100:100 + K],
               genome[200:260] + "N" + genome[261:330], genome[40:190], ls.random_dna(rng, K + 3), genome[:600], "ACGT"]
    fetched = []

    def read_rows(rows):
        fetched.append(np.asarray(rows).size)
        return image[np.asarray(rows, dtype=np.int64)]
    exp = ls.Expected(oracle, read_rows, queries, K, NH, L, W + 4)
    return dict(image=image, real=real, queries=queries, exp=exp, filters=filters, known=known, bits=bits, fetched=fetched)


def oracle_counts(oracle, s, q):
    kmers = oracle.unique_kmers(s["queries"][q], K)
    counts = np.zeros(W + 4, dtype=np.int64)
    if len(kmers):
        for c, m in oracle.search_image(s["image"], s["image"].shape[1], K, NH, L, W + 4, kmers, ORACLE_ALL)[0]:
            counts[c] = m
    return len(kmers), counts


def test_counts_come_from_the_addressed_rows_only(oracle, small):
    exp = small["exp"]
    assert exp.nk.tolist()[3] == 0 and exp.nk[4] == 1 and exp.nk[9] == 0 and exp.nk[5] == (60 - K + 1) + (69 - K + 1)
    assert max(small["fetched"]) <= ls.KMER_CHUNK * NH and sum(small["fetched"]) == sum(r.size for r in exp.rows) - exp.rows[6].size
    for q in range(len(small["queries"])):
        n, counts = oracle_counts(oracle, small, q)
        assert exp.nk[q] == n and np.array_equal(exp.counts[q], counts), q
    assert exp.counts[0, 5] == exp.nk[0] and exp.counts[8, 64] == exp.nk[8] and not exp.counts[:, 65].any()


@pytest.mark.parametrize("t", [1.0, 0.8, 0.05])
def test_every_form_equals_the_oracle_on_the_full_image(oracle, small, t):
    exp, real = small["exp"], small["real"]
    want = []
    for q, seq in enumerate(small["queries"]):
        kmers = oracle.unique_kmers(seq, K)
        if len(kmers):
            hits, _ = oracle.search_image(small["image"], small["image"].shape[1], K, NH, L, W + 4, kmers, float(np.float32(t)))
            want.extend((q, c, m) for c, m in hits if real[c])
    got = ls.hit_records(oracle, exp.counts, exp.nk, real, t)
    assert [tuple(h) for h in got.tolist()] == want and len(want) > 0
    bits = ls.presence_bits(oracle, exp.counts, exp.nk, real, t)
    assert {(q, c) for q, c in np.argwhere(bits).tolist()} == {(q, c) for q, c, _ in want}
    for k in (1, 5, 1024):
        top = []
        for q in range(len(small["queries"])):
            mine = sorted((h for h in want if h[0] == q), key=lambda h: (-h[2], h[1]))[:k]
            top.extend(sorted(mine))
        assert [tuple(h) for h in ls.topk_records(oracle, exp.counts, exp.nk, real, t, k).tolist()] == top, k
    scores = ls.score_matrix(exp.counts, exp.nk, real)
    for q in range(len(small["queries"])):
        n, counts = oracle_counts(oracle, small, q)
        assert np.array_equal(scores[q], np.where(real, counts, 0)), q


def test_known_column_helpers(small):
    rng = np.random.default_rng(611)
    rows = np.array(ls.rows_around(1 << L, 40, offset=40 * 700) + rng.choice(1 << L, size=50).tolist())
    assert {0, (1 << L) - 1, 699, 700, 701} <= set(rows.tolist())
    at = ls.filter_bits_at(small["filters"], rows)
    assert np.array_equal(at, small["bits"][rows][:, small["known"]])
    assert np.array_equal(ls.unpack_columns(small["image"][rows], 64, 2), small["bits"][rows][:, 64:66])
    assert np.array_equal(ls.unpack_columns(small["image"][rows], 5, 290), small["bits"][rows][:, 5:295])
    assert ls.popcount(small["filters"]).tolist() == small["bits"][:, small["known"]].sum(axis=0).tolist()
    assert ls.popcount(small["filters"])[1] == 1 << L and ls.popcount(small["filters"])[2] == 0
    both = ls.popcount(small["filters"][3][None, :] & small["filters"])
    assert both.tolist() == (small["bits"][:, [290]] & small["bits"][:, small["known"]]).sum(axis=0).tolist()
    read = lambda r: small["image"][np.asarray(r, dtype=np.int64)]
    assert np.array_equal(ls.column_sums(read, rows, W), small["bits"][rows].sum(axis=0))
