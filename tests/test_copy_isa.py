"""The kernel of the copy between groups in the gfx950 assembly of copy.hip (`make asm_copy`; no GPU): the unit holds
copy_columns_kernel and nothing else, it does not spill to scratch, it stores with 16-byte stores only, and a 16-byte load
is among its loads."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "copy-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("copy.hip", "copy_kernels.hpp", "copy_plan.hpp", "save_plan.hpp", "insert_plan.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_copy target)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_copy"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    s = open(path).read()
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(starts) == 1, [m.group(1) for m in starts]
    return [s[m.end():s.find(".Lfunc_end", m.end())] for m in starts]


def test_the_unit_holds_the_copy_kernel_only_and_it_uses_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert [name for name, _ in ks] == ["copy_columns_kernel"], sorted(ks)
    for k in ks:
        assert ks[k][1] == 0, k


def test_16_byte_stores_only_and_16_byte_loads(asm):
    for b in bodies(asm):
        stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch|ds)_(?:store|write)_\w+)", b, re.M))
        assert stores == {"global_store_dwordx4"}, sorted(stores)
        loads = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_load_\w+)", b, re.M))
        assert "global_load_dwordx4" in loads and not any(x.startswith("scratch") for x in loads), sorted(loads)
