"""The dense score search's kernels in the gfx950 assembly of scores.hip (`make asm_scores`; no GPU): no instantiation
spills to scratch, every one stores its cells with 16-byte stores only, and the instantiations the compiler emitted are
exactly the ones tests/scores_shapes.py names -- the list test_gpu_scores_shapes.py launches one by one."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

import scores_shapes as ss

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "scores-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("scores.hip", "scores_kernels.hpp", "tile_search.hpp", "score_stage.hpp", "pool_blocks.hpp", "engine_state.hpp", "tuning.hpp", "kernels.hpp", "kmer_device.hpp")      # (the Makefile's asm_scores target)
FAMILIES = ("score_tile_kernel", "score_combine_kernel")


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_scores"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    """{(family, template ints): assembly text of the kernel}"""
    import isa_check
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN5kwage\w+):", s, re.M):
        d = re.match(r"_ZN5kwage(?:\d+_GLOBAL__N_1)?\d+(\w+?)(?:I(.*?)E)?Ev", m.group(1))
        key = (d.group(1), tuple(int(a) for a in re.findall(r"L[ib](\d+)E", d.group(2) or "")))
        out[key] = s[m.end():s.find(".Lfunc_end", m.end())]
    assert set(out) == set(isa_check.kernels(path))           # (the same names tools/isa_check.py reads)
    return out


def test_score_kernels_use_no_scratch(asm):
    import isa_check
    ks = {k: v for k, v in isa_check.kernels(asm).items() if k[0] in FAMILIES}
    assert len(ks) == 30, sorted(ks)
    spilled = {k: scratch for k, (_, scratch) in ks.items() if scratch}
    assert not spilled, spilled
    # and the segment counts of count_kernel this unit instantiates for the combine form
    seg = {k: v for k, v in isa_check.kernels(asm).items() if k[0] == "count_kernel"}
    assert len(seg) == 25 and all(k[1][2] == 1 and not scratch for k, (_, scratch) in seg.items()), sorted(seg)


def test_score_kernels_store_sixteen_bytes_at_a_time(asm):
    for key, body in bodies(asm).items():
        if key[0] not in FAMILIES:
            continue
        stores = re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_\w+)", body, re.M)
        assert stores and set(stores) == {"global_store_dwordx4"}, (key, sorted(set(stores)))
        atomics = re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", body, re.M)
        assert not atomics, (key, atomics)


def test_instantiations_are_the_ones_the_shapes_test_launches(asm):
    found = {k for k in bodies(asm) if k[0] in FAMILIES}
    ledger = set(ss.TILE_SHAPES) | set(ss.COMBINE_SHAPES)
    assert found == ledger, (sorted(found - ledger), sorted(ledger - found))
    assert [ss.planes_for(n) for n in (1, 127, 128, 1023, 1024, 16383, 16384, (1 << 20) - 1, 1 << 20)] == [7, 7, 10, 10, 14, 14, 20, 20, 32]
    assert [ss.planes_for(n) for n in ss.POSITIONS.values()] == list(ss.PLANES)
