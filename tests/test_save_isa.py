"""The save's kernel in the gfx950 assembly of save.hip (`make asm_save`; no GPU): extract_columns_kernel exists in its three
store widths, none of them spills to scratch or holds an atomic, the 16-byte form stores with one 16-byte store and the
dword form with dword stores only; a unit inside one run has a 16-byte load to take."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "save-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("save.hip", "save_kernels.hpp", "save_plan.hpp", "db_writer.hpp", "bloom_files.hpp", "engine_state.hpp", "tuning.hpp", "host.hpp")      # (the Makefile's asm_save target)
WIDTHS = (16, 4, 1)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_save"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    """{(family, template ints): assembly text of the kernel}, under the names tools/isa_check.py reads"""
    import isa_check
    s = open(path).read()
    names = list(isa_check.kernels(path))
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(names) == len(starts)
    return {key: s[m.end():s.find(".Lfunc_end", m.end())] for key, m in zip(names, starts)}


def test_extract_kernel_uses_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert sorted(ks) == sorted(("extract_columns_kernel", (w,)) for w in WIDTHS), sorted(ks)
    spilled = {k: scratch for k, (_, scratch) in ks.items() if scratch}
    assert not spilled, spilled


def test_extract_kernel_holds_no_atomic_and_stores_as_wide_as_its_form_says(asm):
    want = {16: {"global_store_dwordx4"}, 4: {"global_store_dword"}, 1: {"global_store_byte", "global_store_byte_d16_hi"}}      # (d16_hi: the byte in a register's upper half)
    for (name, (width,)), body in bodies(asm).items():
        atomics = re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", body, re.M)
        assert not atomics, (width, atomics)
        stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_\w+)", body, re.M))
        assert stores and stores <= want[width], (width, sorted(stores))
        loads = set(re.findall(r"^\s*((?:global|buffer|flat)_load_\w+)", body, re.M))
        assert {"global_load_dword", "global_load_dwordx4"} <= loads and not any(x.startswith("scratch") for x in loads), (width, sorted(loads))
