"""The top-k contract of include/kwage_amd.h stated plainly, shared by the top-k tests.

- Counts: the CPU oracle (oracle.search_image: C, exact integer counts) per file image; columns it does not report
  count 0; pad columns are not columns (-1 here, below every floor).
- Floor: oracle.query_threshold(t, n) -- the oracle's statement of (unsigned)(t * n), not the library's.
- Selection: real columns with count >= floor, sorted by (count descending, column ascending), cut at k, returned
  ordered by column.  A query without k-mers selects nothing.

A group here is a list of files (first_column, image, num_filter, column_map).  With column_map None the image holds the
file's columns; otherwise the image holds a narrow base block and the file's column j is a copy of base column
column_map[j] -- wide groups whose exact counts cost the oracle one pass over the base."""
import numpy as np

HIT_DTYPE = np.dtype([("query", "<u4"), ("column", "<u4"), ("num_match", "<u4")])
ORACLE_ALL = 1e-12          # a threshold whose floor is 0 for every n: the oracle reports every count


def rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def rand_bits(rng, shape, p):
    """bool array, each bit set with probability ~p (to 1/256), without a float64 array of the same shape."""
    return rng.integers(0, 256, size=shape, dtype=np.uint8) < int(round(p * 256))


def pack_columns(bits, rng, pad_bytes=3):
    """bool [rows, nf] -> uint8 [rows, ceil(nf/8) + pad_bytes] little-endian bit order, garbage in every pad bit."""
    rows, nf = bits.shape
    width = ((nf + 7) // 8 + pad_bytes) * 8
    img = np.empty((rows, width), dtype=bool)
    img[:, :nf] = bits
    img[:, nf:] = rand_bits(rng, (rows, width - nf), 0.5)
    return np.ascontiguousarray(np.packbits(img, axis=1, bitorder="little"))


def column_counts(oracle, files, span, kmer, num_hash, L, kmers):
    """int64 [span]: every column's count for one query's distinct k-mers, -1 on pad columns."""
    counts = np.full(span, -1, dtype=np.int64)
    for first, img, nf, cmap in files:
        base_nf = nf if cmap is None else int(cmap.max()) + 1
        c = np.zeros(base_nf, dtype=np.int64)
        hits, _ = oracle.search_image(img, img.shape[1], kmer, num_hash, L, base_nf, kmers, ORACLE_ALL)
        if hits:
            cols, m = zip(*hits)
            c[np.asarray(cols)] = m
        counts[first:first + nf] = c if cmap is None else c[cmap]
    return counts


def select(counts, floor, k):
    """(columns, counts) of the contract's selection, ordered by column.  O(columns): the k-th largest eligible count v,
    every column above v, the columns at v in ascending order up to k (pinned to a plain sort in test_topk_reference)."""
    cols = np.flatnonzero(counts >= max(int(floor), 0))
    m = counts[cols]
    if cols.size > k:
        v = np.partition(m, cols.size - k)[cols.size - k]
        above = cols[m > v]
        at = cols[m == v][:k - above.size]
        cols = np.sort(np.concatenate([above, at]))
    return cols, counts[cols]


def expected_hits(oracle, per_query, t, k):
    """per_query: [(n, counts)] in batch order -> (HIT_DTYPE records ordered by (query, column), floors)."""
    parts, floors = [], []
    for q, (n, counts) in enumerate(per_query):
        f = oracle.query_threshold(float(np.float32(t)), n)
        floors.append(f)
        if n == 0:
            continue
        cols, m = select(counts, f, k)
        rec = np.empty(cols.size, dtype=HIT_DTYPE)
        rec["query"], rec["column"], rec["num_match"] = q, cols, m
        parts.append(rec)
    return (np.concatenate(parts) if parts else np.empty(0, HIT_DTYPE)), np.asarray(floors, dtype=np.uint32)


def cut_threshold_hits(hits, k):
    """A threshold search's records cut to each query's first k under (num_match descending, column ascending),
    returned ordered by (query, column)."""
    if hits.size == 0:
        return hits.copy()
    q, c, m = (hits[f].astype(np.int64) for f in ("query", "column", "num_match"))
    order = np.lexsort((c, -m, q))
    qs = q[order]
    start = np.searchsorted(qs, qs, side="left")
    kept = order[(np.arange(qs.size) - start) < k]
    kept = kept[np.lexsort((c[kept], q[kept]))]
    return hits[kept].copy()


def assert_hits_equal(got, exp, what):
    got = np.asarray(got).astype(HIT_DTYPE)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return
    bad = [q for q in sorted(set(exp["query"].tolist()) | set(got["query"].tolist()))
           if not np.array_equal(got[got["query"] == q], exp[exp["query"] == q])]
    q = bad[0] if bad else None
    raise AssertionError("%s: %d vs %d records, %d queries differ, first %s: got %s expected %s" % (
        what, got.size, exp.size, len(bad), q,
        got[got["query"] == q][:6].tolist() if q is not None else None,
        exp[exp["query"] == q][:6].tolist() if q is not None else None))
