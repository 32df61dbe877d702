"""The filter set's kernels in the gfx950 assembly of filterset.hip (`make asm_filterset`; no GPU): the unit holds
exactly its own five kernels -- none of the score kernels, which stay scores.hip's (tests/test_scores_isa.py) -- and none
of them spills to scratch."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
ASM = os.path.join(ROOT, "kwage_amd", "lib", "asm", "filterset-hip-amdgcn-amd-amdhsa-gfx950.s")
SOURCES = ("filterset.hip", "filterset_kernels.hpp", "score_stage.hpp", "pool_blocks.hpp", "engine_state.hpp", "tuning.hpp")      # (the Makefile's asm_filterset target)
KERNELS = {"column_bits_kernel", "filter_count_kernel", "filter_scan_kernel", "filter_expand_kernel", "identity_rows_kernel"}


@pytest.fixture(scope="module")
def asm():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < newest:
        subprocess.check_call(["make", "-C", CSRC, "asm_filterset"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ASM


def test_the_unit_holds_its_own_kernels_only(asm):
    import isa_check
    ks = isa_check.kernels(asm)
    assert {name for name, _ in ks} == KERNELS, sorted(ks)
    assert all(args == () for _, args in ks)             # (no templates: nothing of kernels.hpp is instantiated here)


def test_filterset_kernels_use_no_scratch(asm):
    import isa_check
    spilled = {k: scratch for k, (_, scratch) in isa_check.kernels(asm).items() if scratch}
    assert not spilled, spilled
