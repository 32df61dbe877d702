"""The compaction's kernel in the gfx950 assembly of compact.hip (`make asm_compact`; no GPU): the unit holds
compact_rows_kernel and nothing else, it does not spill to scratch and holds no atomic, it stores with 16-byte stores
only, the ordering between a segment's loads and its stores is a workgroup barrier that every path through the segment loop
passes, and a unit inside one run has a 16-byte load to take."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "compact-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("compact.hip", "compact_kernels.hpp", "compact_plan.hpp", "save_plan.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_compact target)


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_compact"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def body(path):
    s = open(path).read()
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(starts) == 1, [m.group(1) for m in starts]
    return s[starts[0].end():s.find(".Lfunc_end", starts[0].end())]


def test_the_unit_holds_the_compaction_kernel_only_and_it_uses_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert sorted(ks) == [("compact_rows_kernel", ())], sorted(ks)
    assert ks[("compact_rows_kernel", ())][1] == 0


def test_no_atomic_and_16_byte_stores_only(asm):
    b = body(asm)
    atomics = re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", b, re.M)
    assert not atomics, atomics
    stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch|ds)_(?:store|write)_\w+)", b, re.M))
    assert stores == {"global_store_dwordx4"}, sorted(stores)
    loads = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_load_\w+)", b, re.M))
    assert {"global_load_dword", "global_load_dwordx4"} <= loads and not any(x.startswith("scratch") for x in loads), sorted(loads)


def test_a_barrier_stands_between_the_loads_and_the_store(asm):
    lines = [ln.strip() for ln in body(asm).splitlines()]
    barriers = [i for i, ln in enumerate(lines) if ln.startswith("s_barrier")]
    stores = [i for i, ln in enumerate(lines) if ln.startswith("global_store_dwordx4")]
    loads = [i for i, ln in enumerate(lines) if ln.startswith("global_load_dword")]
    assert len(barriers) == 1 and len(stores) == 1          # one place where the workgroup meets, one place that writes
    assert max(loads) < barriers[0] < stores[0]             # in program order: every load, the barrier, the store
    # all outstanding loads have returned when the wave arrives: a vmcnt(0) wait between the last load and the barrier
    assert any(ln.startswith("s_waitcnt") and "vmcnt(0)" in ln for ln in lines[max(loads):barriers[0]])
