"""The presence search's kernels in the gfx950 assembly of presence.hip (`make asm_presence`; no GPU): no kernel spills
to scratch, the tile, combine and AND kernels store their bits with 16-byte stores only and hold no atomic, and the
kernels the compiler emitted are exactly the ones tests/presence_shapes.py names -- the list
test_gpu_presence_shapes.py launches one by one."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import presence_shapes as ps

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "presence-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("presence.hip", "presence_kernels.hpp", "tile_search.hpp", "pool_blocks.hpp", "engine_state.hpp", "tuning.hpp", "kernels.hpp", "kmer_device.hpp")      # (the Makefile's asm_presence target)
BIT_FAMILIES = ("presence_tile_kernel", "presence_combine_kernel", "presence_and_kernel")
FAMILIES = BIT_FAMILIES + ("presence_popcount_kernel",)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_presence"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    """{(family, template ints): assembly text of the kernel}, under the names tools/isa_check.py reads"""
    import isa_check
    s = open(path).read()
    names = list(isa_check.kernels(path))
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(names) == len(starts)                      # (isa_check walks the same labels in the same order)
    return {key: s[m.end():s.find(".Lfunc_end", m.end())] for key, m in zip(names, starts)}


def test_presence_kernels_use_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    mine = {k: v for k, v in ks.items() if k[0] in FAMILIES}
    assert len(mine) == 25 + 5 + 1 + 1, sorted(mine)
    spilled = {k: scratch for k, (_, scratch) in mine.items() if scratch}
    assert not spilled, spilled
    # and the segment counts of count_kernel this unit instantiates for the combine form
    seg = {k: v for k, v in ks.items() if k[0] == "count_kernel"}
    assert len(seg) == 25 and all(k[1][2] == 1 and not scratch for k, (_, scratch) in seg.items()), sorted(seg)


def test_presence_kernels_store_sixteen_bytes_at_a_time(asm):
    seen = 0
    for key, body in bodies(asm).items():
        if key[0] not in BIT_FAMILIES:
            continue
        seen += 1
        stores = re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_\w+)", body, re.M)
        assert stores and set(stores) == {"global_store_dwordx4"}, (key, sorted(set(stores)))
        atomics = re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", body, re.M)
        assert not atomics, (key, atomics)
    assert seen == 31
    # the popcount kernel: one word per query, summed through LDS without an atomic
    body = bodies(asm)[("presence_popcount_kernel", ())]
    assert not re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", body, re.M)


def test_instantiations_are_the_ones_the_shapes_test_launches(asm):
    found = set(bodies(asm))
    ledger = set(ps.TILE_SHAPES) | set(ps.COMBINE_SHAPES) | set(ps.PLAIN_SHAPES) | set(ps.SEG_COUNT_SHAPES)
    assert len(ps.TILE_SHAPES) == 25 and len(ps.COMBINE_SHAPES) == 5 and len(ps.SEG_COUNT_SHAPES) == 25
    assert found == ledger, (sorted(found - ledger), sorted(ledger - found))
    assert [ps.planes_for(n) for n in (1, 127, 128, 1023, 1024, 16383, 16384, (1 << 20) - 1, 1 << 20)] == [7, 7, 10, 10, 14, 14, 20, 20, 32]
    assert [ps.planes_for(n) for n in ps.POSITIONS.values()] == list(ps.PLANES)
