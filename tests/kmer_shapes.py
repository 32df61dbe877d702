"""The k-mer stage (kmer_kernel + kmer_finish_kernel; engine.hip launch_kmer_kernels / batch_prepare, kernels.hpp
kmer_body) stated as data: the form a batch is launched in, and the table of batches that together reach every form and
both sides of every edge between two forms.  k-mer positions of a query: P = len - k + 1.

- threads(max_pos), lds_slots(max_pos): the workgroup size and the dynamic-LDS table of a launch, both sized by the
  batch's longest query (launch_kmer_kernels).
- table_log2(P), in_lds(P, slots), chunks(P, slots): per query -- its set has 2^table_log2(P) slots; it lies in LDS when
  that fits the launch's table, else in a global table that ceil(P / KM_CHUNK) workgroups work on together (MULTI), and
  the batch then runs kmer_finish_kernel.
- form(max_pos): Form(threads, slots, chunks of the longest query, finish kernel or not).
- UNREACHABLE: the branch of kmer_kernel the dispatch compiles but no input takes, with the reason.
- BATCHES: what test_gpu_kmer_shapes.py runs -- one batch per longest query P, each with the form it must land in.
  test_kmer_shapes_ledger.py checks on CPU that the constants here are the sources' and that the batches reach
  everything."""
from collections import namedtuple

KM_THREADS = 256            # kernels.hpp
KM_LDS_SLOTS = 4096         # kernels.hpp
KM_CHUNK = 1024             # kernels.hpp
WG64_MAX_POS = 192          # engine.hip launch_kmer_kernels: 64 threads up to here
WG128_MAX_POS = 768         # engine.hip launch_kmer_kernels: 128 threads up to here
MIN_SLOTS = 64              # engine.hip launch_kmer_kernels; 2^MIN_TABLE_LOG2
MIN_TABLE_LOG2 = 6          # kernels.hpp table_log2, engine.hip host_table_log2

WORKGROUP_SIZES = (64, 128, KM_THREADS)


def threads(max_pos):
    return 64 if max_pos <= WG64_MAX_POS else 128 if max_pos <= WG128_MAX_POS else KM_THREADS


def lds_slots(max_pos):
    """The smallest power of two >= 2 max_pos, at least MIN_SLOTS, at most KM_LDS_SLOTS."""
    slots = MIN_SLOTS
    while slots < KM_LDS_SLOTS and slots < 2 * max_pos:
        slots *= 2
    return slots


def table_log2(npos):
    lg = MIN_TABLE_LOG2
    while (1 << lg) < 2 * npos:
        lg += 1
    return lg


def in_lds(npos, slots):
    return (1 << table_log2(npos)) <= slots


def chunks(npos, slots):
    """Workgroups on a query of npos > 0 positions in a launch with `slots` LDS slots."""
    return 1 if in_lds(npos, slots) or npos <= KM_CHUNK else -(-npos // KM_CHUNK)


Form = namedtuple("Form", "threads slots chunks finish")


def form(max_pos):
    slots = lds_slots(max_pos)
    return Form(threads(max_pos), slots, chunks(max_pos, slots), not in_lds(max_pos, slots))


# Compiled, never taken.
UNREACHABLE = {
    "kmer_kernel: `else if(npos <= KM_CHUNK)`, one workgroup on a query's own global set":
        "taken for a query whose set does not fit the launch's LDS table and that has P <= KM_CHUNK = 1024 "
        "positions; but the launch's table holds the set of the batch's longest query up to KM_LDS_SLOTS = 4096 slots, so a "
        "set that does not fit has more than 4096 slots: P > 2048",
}

# ---- the batch table -----------------------------------------------------------------------------------------------------
# The edges between forms, as the last P of the lower side.
THREAD_EDGES = (WG64_MAX_POS, WG128_MAX_POS)
SLOT_EDGES = (32, 64, 128, 256, 512, 1024)          # 2 P = 64 ... 2048 slots; the table above is 128 ... 4096
MULTI_EDGE = KM_LDS_SLOTS // 2                      # 2048: the last query with an LDS set

Batch = namedtuple("Batch", "max_pos form")

BATCHES = [
    Batch(1, Form(64, 64, 1, False)),
    Batch(32, Form(64, 64, 1, False)),
    Batch(33, Form(64, 128, 1, False)),
    Batch(64, Form(64, 128, 1, False)),
    Batch(65, Form(64, 256, 1, False)),
    Batch(128, Form(64, 256, 1, False)),
    Batch(129, Form(64, 512, 1, False)),
    Batch(192, Form(64, 512, 1, False)),
    Batch(193, Form(128, 512, 1, False)),
    Batch(256, Form(128, 512, 1, False)),
    Batch(257, Form(128, 1024, 1, False)),
    Batch(512, Form(128, 1024, 1, False)),
    Batch(513, Form(128, 2048, 1, False)),
    Batch(768, Form(128, 2048, 1, False)),
    Batch(769, Form(256, 2048, 1, False)),
    Batch(1024, Form(256, 2048, 1, False)),
    Batch(1025, Form(256, 4096, 1, False)),
    Batch(2048, Form(256, 4096, 1, False)),
    Batch(2049, Form(256, 4096, 3, True)),           # last chunk: one position
    Batch(3072, Form(256, 4096, 3, True)),           # whole chunks
    Batch(3073, Form(256, 4096, 4, True)),           # last chunk: one position
    Batch(4097, Form(256, 4096, 5, True)),           # last chunk: one position
    Batch(5000, Form(256, 4096, 5, True)),           # last chunk: 904 positions, its last tile 136 of 256
]
MAX_POS = [b.max_pos for b in BATCHES]
