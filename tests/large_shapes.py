"""References for groups too large to mirror on the host (tests/test_gpu_large_offsets.py), and their CPU check
(tests/test_large_shapes_reference.py).  Every expected value comes from one of two sources, never from a search:

  addressed rows   a query's rows are oracle.unique_kmers + oracle.row_indices; `read_rows(rows)` (Group.read_rows, or a
                   host image's rows in the CPU test) fetches only those; numpy ANDs each k-mer's num_hash rows and sums
                   over the k-mers: num_match of every column (column_counts).  The four search forms follow from that
                   vector: hit_records, presence_bits, topk_records, score_matrix.
  known columns    filters the test inserted itself, uint8 [n, 2^L / 8] on the host: bit r of filter c is
                   (F[c, r >> 3] >> (r & 7)) & 1 (filter_bits_at), a column's set bits are the filter's popcount.

A group here is anything with read_rows(rows) -> uint8 [len(rows), >= ceil(span / 8)]."""
import numpy as np

from topk_reference import HIT_DTYPE, expected_hits

POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)
KMER_CHUNK = 248            # k-mers reduced per step: below 256, so a step's column sums fit a byte


def random_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def mutated(seq, every, start=11):
    s = list(seq)
    for p in range(start, len(s), every):
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def popcount(a):
    """Set bits of a uint8 array, along its last axis."""
    return POP8[a].sum(axis=-1, dtype=np.int64)


def filter_bits_at(filters, rows):
    """bool [len(rows), n]: bit rows[i] of every filter (uint8 [n, bytes], LSB first)."""
    rows = np.asarray(rows, dtype=np.int64)
    return ((filters[:, rows >> 3] >> (rows & 7).astype(np.uint8)[None, :]) & 1).T.astype(bool)


def unpack_columns(packed, first, n):
    """bool [rows, n]: columns first .. first + n - 1 of packed rows (uint8 [rows, bytes], LSB first)."""
    b0, b1 = first // 8, (first + n + 7) // 8
    return np.unpackbits(packed[:, b0:b1], axis=1, bitorder="little")[:, first - 8 * b0:first - 8 * b0 + n].astype(bool)


def query_rows(oracle, seq, k, num_hash, L):
    """uint32 [distinct k-mers, num_hash]: the rows a query addresses, k-mer by k-mer."""
    return oracle.row_indices(oracle.unique_kmers(seq, k), k, num_hash, L)


def column_sums(read_rows, rows, span):
    """int64 [span]: over the listed rows, how many have each column's bit set."""
    total = np.zeros(span, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.uint32)
    for i in range(0, rows.size, KMER_CHUNK):
        got = read_rows(rows[i:i + KMER_CHUNK])
        total += np.unpackbits(got, axis=1, bitorder="little")[:, :span].sum(axis=0, dtype=np.uint8)
    return total


def column_counts(read_rows, rows, span):
    """int64 [span]: num_match of every column for one query's rows [n, num_hash] -- AND over a k-mer's rows, then the
    sum over the k-mers."""
    total = np.zeros(span, dtype=np.int64)
    nb = (span + 7) // 8
    for i in range(0, rows.shape[0], KMER_CHUNK):
        part = rows[i:i + KMER_CHUNK]
        got = read_rows(part.reshape(-1))[:, :nb].reshape(part.shape[0], part.shape[1], nb)
        hit = np.bitwise_and.reduce(got, axis=1)
        total += np.unpackbits(hit, axis=1, bitorder="little")[:, :span].sum(axis=0, dtype=np.uint8)
    return total


class Expected:
    """num_match of every column for every query of a batch, from the rows the batch addresses."""

    def __init__(self, oracle, read_rows, queries, k, num_hash, L, span):
        self.rows, self.counts = [], np.zeros((len(queries), span), dtype=np.int64)
        done = {}
        for q, seq in enumerate(queries):
            if seq not in done:
                r = query_rows(oracle, seq, k, num_hash, L)
                done[seq] = (r, column_counts(read_rows, r, span) if r.shape[0] else np.zeros(span, dtype=np.int64))
            self.rows.append(done[seq][0])
            self.counts[q] = done[seq][1]
        self.nk = np.array([r.shape[0] for r in self.rows], dtype=np.uint32)

    def all_rows(self):
        return np.concatenate([r.reshape(-1) for r in self.rows]).astype(np.int64)


def floors(oracle, nk, t):
    return np.array([oracle.query_threshold(float(np.float32(t)), int(n)) for n in nk], dtype=np.int64)


def presence_bits(oracle, counts, nk, real, t):
    """bool [n, span]: the cells a threshold search reports."""
    return real[None, :] & (counts >= floors(oracle, nk, t)[:, None]) & (nk[:, None] > 0)


def hit_records(oracle, counts, nk, real, t):
    """HIT_DTYPE records in (query, column) order."""
    q, c = np.nonzero(presence_bits(oracle, counts, nk, real, t))
    rec = np.empty(q.size, dtype=HIT_DTYPE)
    rec["query"], rec["column"], rec["num_match"] = q, c, counts[q, c]
    return rec


def topk_records(oracle, counts, nk, real, t, k):
    """(-num_match, column) cut at k, listed by (query, column): topk_reference's selection on the masked counts."""
    return expected_hits(oracle, [(int(nk[q]), np.where(real, counts[q], -1)) for q in range(len(nk))], t, k)[0]


def score_matrix(counts, nk, real):
    return np.where(real[None, :] & (nk[:, None] > 0), counts, 0).astype(np.uint32)


def rows_around(nrows, stride, offset=1 << 32):
    """The first row, the last, and the rows on both sides of byte `offset` of a matrix of `stride` bytes per row."""
    edge = offset // stride
    return sorted({0, 1, nrows - 2, nrows - 1} | {r for r in (edge - 1, edge, edge + 1) if 0 <= r < nrows})
