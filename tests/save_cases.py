"""The cases of tests/test_gpu_save.py as data: what is inserted into a fresh group, what is retired, and which of the
surviving columns are saved in what order.  Filters are `.bloom` files with random bits and run accession SRR<j + 1>;
filter j of a case becomes column j of the group (the first insert of a fresh group starts at column 0).

    L        log2 of the filter length (rows of the group)
    calls    filters per kwage_group_insert_bloom_files call, in order
    retire   filters withdrawn after the inserts
    order    "ascending" | "reverse" | "permutation": the order the survivors are listed in
    runs     the runs the list must fold into (stats.runs)"""
import numpy as np

K, NH = 21, 2


def survivors(case):
    n = sum(case["calls"])
    keep = [j for j in range(n) if j not in set(case["retire"])]
    if case["order"] == "reverse":
        keep = keep[::-1]
    elif case["order"] == "permutation":
        keep = [keep[i] for i in np.random.default_rng(case["seed"]).permutation(len(keep)).tolist()]
    return keep


def count_runs(cols):
    return 1 + sum(1 for a, b in zip(cols, cols[1:]) if b != a + 1)


CASES = {
    # 1. one column: out_slice is 1 byte with 7 zero pad bits; L = 3 is one byte per filter
    "one_column": dict(L=10, calls=[1], retire=[], order="ascending", runs=1),
    "one_column_L5": dict(L=5, calls=[1], retire=[], order="ascending", runs=1),
    "one_column_L3": dict(L=3, calls=[1], retire=[], order="ascending", runs=1),
    # 2. inserted one per call: n % 8 = 5, n % 32 = 5
    "one_at_a_time": dict(L=10, calls=[1] * 37, retire=[], order="ascending", runs=1),
    # 3. runs that begin and end on both sides of source and destination dword boundaries
    "retired": dict(L=10, calls=[100], retire=[0, 31, 32, 33, 63, 64, 99], order="ascending", runs=3),
    "retired_L5": dict(L=5, calls=[100], retire=[0, 31, 32, 33, 63, 64, 99], order="ascending", runs=3),
    # 4. every second one retired: 35 runs of length 1
    "alternate": dict(L=10, calls=[70], retire=list(range(1, 70, 2)), order="ascending", runs=35),
    # 6. reordered lists
    "reverse": dict(L=10, calls=[130], retire=[], order="reverse", runs=130),
    "permutation": dict(L=10, calls=[130], retire=[], order="permutation", seed=6, runs=None),
    # 7. wide rows at L = 5: out_slice 256 (the 16-byte path), 261 (row starts off dword boundaries), 261 again with
    #    another tail (2048 + 33 columns: one bit into the second dword behind the 16-byte units)
    "wide_2048": dict(L=5, calls=[2048], retire=[], order="ascending", runs=1),
    "wide_2088": dict(L=5, calls=[2048, 40], retire=[], order="ascending", runs=1),
    "wide_2081": dict(L=5, calls=[2081], retire=[], order="ascending", runs=1),
    # (the dword path: out_slice 260, and 12 with a short last unit)
    "wide_2080": dict(L=5, calls=[2080], retire=[], order="ascending", runs=1),
    "dwords_96": dict(L=10, calls=[96], retire=[], order="ascending", runs=1),
}

# 8. staged chunks on the "retired" groups: 93 columns, out_slice 12.  name -> (case, staging_bytes, chunks)
STAGED = {
    "two_chunks": ("retired", 512 * 12, 2),
    "four_chunks": ("retired", 256 * 12, 4),
    "last_chunk_of_one_row": ("retired", 341 * 12, 4),          # 1024 = 3 * 341 + 1
    "a_byte_short_of_two_rows": ("retired", 2 * 12 - 1, 1024),
    "one_row_per_chunk_L5": ("retired_L5", 12, 32),
    "less_than_a_row_L5": ("retired_L5", 1, 32),
}
