"""The export's kernel in the gfx950 assembly of export.hip (`make asm_export`; no GPU): the unit holds export_filters_kernel
in the one shape export.hip launches and nothing else, it does not spill to scratch and holds no atomic, a unit inside one
run has a 16-byte load to take, global memory is written with dword and byte stores only, and one workgroup barrier stands
between the matrix loads and the stores."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "export-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("export.hip", "export_kernels.hpp", "export_plan.hpp", "save_plan.hpp", "save_records.hpp", "transpose_tile.hpp", "engine_state.hpp",
           "tuning.hpp", "host.hpp")      # (the Makefile's asm_export target)
SHAPES = ((16, 8),)                       # export.hip's ExportTile: TransposeTile<16, 8>


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_export"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def bodies(path):
    """{(family, template ints): assembly text of the kernel}, under the names tools/isa_check.py reads"""
    import isa_check
    s = open(path).read()
    names = list(isa_check.kernels(path))
    starts = list(re.finditer(r"^(_ZN5kwage\w+):", s, re.M))
    assert len(names) == len(starts)
    return {key: s[m.end():s.find(".Lfunc_end", m.end())] for key, m in zip(names, starts)}


def test_the_launched_shape_is_in_the_source():
    src = open(os.path.join(CSRC, "export.hip")).read()
    m = re.search(r"using ExportTile = TransposeTile<(\d+), (\d+)>;", src)
    assert m and (int(m.group(1)), int(m.group(2))) in SHAPES
    assert src.count("export_filters_kernel<") == 1          # one launch site, shaped by ExportTile


def test_the_unit_holds_the_export_kernel_only_and_it_uses_no_scratch(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert sorted(ks) == sorted(("export_filters_kernel", s) for s in SHAPES), sorted(ks)
    spilled = {k: scratch for k, (_, scratch) in ks.items() if scratch}
    assert not spilled, spilled


def test_no_atomic_a_16_byte_load_and_dword_and_byte_stores_only(asm):
    for key, body in bodies(asm).items():
        atomics = re.findall(r"^\s*((?:global|buffer|flat|ds)_atomic\w+)", body, re.M)
        assert not atomics, (key, atomics)
        stores = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_\w+)", body, re.M))
        assert {"global_store_dword"} <= stores <= {"global_store_dword", "global_store_byte", "global_store_byte_d16_hi"}, (key, sorted(stores))      # (d16_hi: the byte in a register's upper half)
        loads = set(re.findall(r"^\s*((?:global|buffer|flat|scratch)_load_\w+)", body, re.M))
        assert {"global_load_dword", "global_load_dwordx4"} <= loads and not any(x.startswith("scratch") for x in loads), (key, sorted(loads))
        assert re.search(r"^\s*global_load_dwordx4 .* nt\b", body, re.M), key          # the unit's own (nontemporal) 16-byte load, not the run table's


def test_one_barrier_between_the_matrix_loads_and_the_stores(asm):
    for key, body in bodies(asm).items():
        lines = [ln.strip() for ln in body.splitlines()]
        barriers = [i for i, ln in enumerate(lines) if ln.startswith("s_barrier")]
        stores = [i for i, ln in enumerate(lines) if ln.startswith("global_store_")]
        loads = [i for i, ln in enumerate(lines) if ln.startswith("global_load_")]
        assert len(barriers) == 1, (key, barriers)
        assert max(loads) < barriers[0] < min(stores), key
        # the fast path: 32 dword stores with no branch between them
        run = best = 0
        for ln in lines[barriers[0]:]:
            if ln.startswith("global_store_dword "):
                run += 1
                best = max(best, run)
            elif ln.startswith(("s_cbranch", "s_branch")) or ln.endswith(":"):
                run = 0
        assert best >= 32, (key, best)
