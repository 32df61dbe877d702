"""The fold's kernel in the gfx950 assembly of fold.hip (`make asm_fold`; no GPU): the unit holds fold_rows_kernel in its
three instantiations and nothing else, none of them spills to scratch, they store with 16-byte stores only, and a 16-byte
load is among their loads."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "fold-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("fold.hip", "fold_kernels.hpp", "fold_plan.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_fold target)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_fold"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    s = open(path).read()
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(starts) == 3, [m.group(1) for m in starts]
    return [s[m.end():s.find(".Lfunc_end", m.end())] for m in starts]


def test_the_unit_holds_the_three_fold_kernels_only_and_none_uses_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert sorted(ks) == [("fold_rows_kernel", (j,)) for j in (1, 2, 3)], sorted(ks)
    for j in (1, 2, 3):
        assert ks[("fold_rows_kernel", (j,))][1] == 0, j


def test_16_byte_stores_only_and_16_byte_loads(asm):
    for b in bodies(asm):
        stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch|ds)_(?:store|write)_\w+)", b, re.M))
        assert stores == {"global_store_dwordx4"}, sorted(stores)
        loads = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_load_\w+)", b, re.M))
        assert "global_load_dwordx4" in loads and not any(x.startswith("scratch") for x in loads), sorted(loads)
