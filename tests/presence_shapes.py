"""The ledger of the presence search's kernel shapes, shared by test_gpu_presence_shapes.py (which launches every one of
them on the GPU) and test_presence_isa.py (which compares the list with what the compiler emitted, without a GPU).

A batch whose longest query has `positions` k-mer positions is counted in planes_for(positions) counter planes; the
hash count of the group picks the second template argument.  force_segs = 1 keeps the unsegmented forms -- the tile
kernel below t = 1, presence_and_kernel (no template shape: the hash count is a launch argument) at t = 1 --
force_segs = 3 the segmented one (count_kernel<seg planes, nh, SEG> + presence_combine_kernel<planes>)."""

PLANES = (7, 10, 14, 20, 32)
HASHES = (1, 2, 3, 4, 5)
# the longest query of the batch that reaches each counter width (the last: >= 2^20 positions, on a narrow group)
POSITIONS = {7: 100, 10: 1000, 14: 10000, 20: 100000, 32: (1 << 20) + 1500}
FORCED_SEGS = 3
AND_NAME = "presence_and_kernel"


def planes_for(max_count):
    """The narrowest instantiated counter width holding counts up to max_count (engine.hip planes_for)."""
    return next(p for p in PLANES if max_count < (1 << p))


def tile_name(p, nh):
    return "presence_tile_kernel<%d,%d>" % (p, nh)


def combine_name(p, nh, positions, segs=FORCED_SEGS):
    seg_kmers = -(-positions // segs)
    return "count_kernel<%d,%d>+presence_combine_kernel<%d>" % (planes_for(seg_kmers), nh, p)


# every instantiation the GPU test launches: (family, template arguments)
TILE_SHAPES = [("presence_tile_kernel", (p, nh)) for p in PLANES for nh in HASHES]
COMBINE_SHAPES = [("presence_combine_kernel", (p,)) for p in PLANES]
PLAIN_SHAPES = [("presence_and_kernel", ()), ("presence_popcount_kernel", ())]
# count_kernel's SEG form, which the unit instantiates for the segments: (planes, nh, SEG = 1)
SEG_COUNT_SHAPES = [("count_kernel", (p, nh, 1)) for p in PLANES for nh in HASHES]
