"""The kernel of the union of columns in the gfx950 assembly of union.hip (`make asm_union`; no GPU): the unit holds
union_columns_kernel and nothing else, it does not spill to scratch, it stores with 16-byte stores only, and
tools/isa_check.py's run count shows eight 16-byte loads requested together before the first wait -- the eight entries of a
round, each of which says which source dword the round requests next."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "union-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("union.hip", "union_kernels.hpp", "union_plan.hpp", "copy_plan.hpp", "save_plan.hpp", "insert_plan.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_union target)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_union"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    s = open(path).read()
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(starts) == 1, [m.group(1) for m in starts]
    return [s[m.end():s.find(".Lfunc_end", m.end())] for m in starts]


def test_the_unit_holds_the_union_kernel_only_and_it_uses_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert [name for name, _ in ks] == ["union_columns_kernel"], sorted(ks)
    for k in ks:
        assert ks[k][1] == 0, k


def test_16_byte_stores_only(asm):
    for b in bodies(asm):
        stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch|ds)_(?:store|write)_\w+)", b, re.M))
        assert stores == {"global_store_dwordx4"}, sorted(stores)


def test_eight_loads_are_requested_together(asm):
    import isa_check
    (runs, _), = isa_check.kernels(asm).values()
    assert max(runs) == 8, dict(runs)
