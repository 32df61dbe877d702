"""The kernels of the overlap matrix in the gfx950 assembly of overlap.hip (`make asm_overlap`; no GPU): the unit holds
overlap_mfma_kernel and overlap_combine_kernel and nothing else, neither spills to scratch, the products are integer
matrix instructions (v_mfma_i32_*) with no floating-point one beside them, and every global store is of one width."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "overlap-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("overlap.hip", "overlap_kernels.hpp", "overlap_plan.hpp", "transpose_tile.hpp", "copy_plan.hpp", "save_plan.hpp", "insert_plan.hpp",
           "pool_blocks.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_overlap target)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_overlap"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    s = open(path).read()
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(starts) == 2, [m.group(1) for m in starts]
    return {m.group(1): s[m.end():s.find(".Lfunc_end", m.end())] for m in starts}


def test_the_unit_holds_the_two_kernels_and_they_use_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert sorted(name for name, _ in ks) == ["overlap_combine_kernel", "overlap_mfma_kernel"], sorted(ks)
    for k in ks:
        assert ks[k][1] == 0, k


def test_integer_matrix_instructions_only(asm):
    b = bodies(asm)
    main = next(v for k, v in b.items() if "overlap_mfma_kernel" in k)
    assert len(re.findall(r"^\s*v_mfma_i32_", main, re.M)) >= 1
    for body in b.values():
        assert not re.findall(r"^\s*v_mfma_f32_", body, re.M)


def test_global_stores_are_of_one_width(asm):
    stores = set()
    for body in bodies(asm).values():
        stores |= set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_\w+)", body, re.M))
    assert len(stores) == 1, sorted(stores)
