"""The ledger of tests/search_shapes.py against the gfx950 assembly of engine.hip (no GPU): the case table of
test_gpu_search_shapes.py launches every gather-kernel instantiation the compiler emitted, every instantiation the ledger
names exists, and every name the search can report (search_plan.hpp format_search_name) is understood.  An instantiation added without a case, a case lost,
or an instantiation left behind that nothing launches fails here, naming it."""
import os
import re
import sys

from conftest import ROOT

import search_shapes as ss

sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "kwage_amd", "csrc")
SOURCES = ("engine.hip", "engine_state.hpp", "tuning.hpp", "kernels.hpp", "search_plan.hpp", "kmer_device.hpp")      # (the Makefile's asm target)


def gather_instantiations():
    import isa_check
    asm = isa_check.ASM
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(asm) or os.path.getmtime(asm) < newest:
        isa_check.build()
    return {k for k in isa_check.kernels(asm) if k[0] in ss.GATHER_FAMILIES}


def fmt(keys):
    return ", ".join(sorted("%s<%s>" % (f, ",".join(map(str, a))) for f, a in keys))


def test_cases_launch_every_gather_instantiation():
    asm = gather_instantiations()
    assert len(asm) > 200, len(asm)
    covered = set().union(*(ss.launched(c.name) for c in ss.CASES))
    missing = asm - covered - set(ss.UNREACHABLE)
    assert not missing, "instantiations no case launches: " + fmt(missing)
    claimed = covered | set(ss.UNREACHABLE)
    assert claimed <= asm, "instantiations the ledger names but the assembly lacks: " + fmt(claimed - asm)
    assert not covered & set(ss.UNREACHABLE), fmt(covered & set(ss.UNREACHABLE))
    # every family has its own test in the GPU file: each test checks that it reached all of its family's instantiations
    for c in ss.CASES:
        assert c.test in {"and_narrow", "and_screen", "and_walk", "and_band_walk", "and_kernel", "count_screen", "count_walk_trunc",
                          "count_walk_pf", "count_kernel", "count_segments", "count_narrow"}, c
        assert c.batch in ss.BATCH_MAX_POS, c


def test_every_printable_name_is_understood():
    src = open(os.path.join(CSRC, "search_plan.hpp")).read()
    formats = set(re.findall(r'snprintf\(out, n, "([^"]*)"', src.split("inline void format_search_name(")[1]))
    assert formats == set(ss.FORMATS), (formats ^ set(ss.FORMATS))
    asm = gather_instantiations()
    for name in ss.printable_names():
        got = ss.launched(name)
        assert got and got <= asm, (name, fmt(got - asm))
    assert {c.name for c in ss.CASES} <= set(ss.printable_names()), {c.name for c in ss.CASES} - set(ss.printable_names())
    for bad in ("count_walk_kernel<14,2,pf>", "count_walk_kernel<10,2,pf,8>", "count_kernel<20,1>+segments->14",
                "and_kernel<4,8>", "count_kernel<7,1,0>", "kmer_kernel"):
        try:
            ss.launched(bad)
        except ValueError:
            continue
        raise AssertionError("launched() accepted %r" % bad)


def test_case_names_follow_the_dispatch_rules():
    """The names in CASES restate search_plan.hpp's choices; pinned here where they are plain arithmetic (test_search_plan.py
    runs the plan itself on every case)."""
    assert [ss.planes_for(n) for n in (1, 127, 128, 1023, 1024, 16383, 16384, (1 << 20) - 1, 1 << 20)] == [7, 7, 10, 10, 14, 14, 20, 20, 32]
    for c in ss.CASES:
        if c.test == "count_screen":
            p, up = int(c.name.split("<")[1].split(",")[0]), int(c.name.rsplit("<", 1)[1][:-1])
            assert p == ss.planes_for(ss.BATCH_MAX_POS[c.batch]) and (up == 14) == (ss.BATCH_MAX_POS[c.batch] > 8192), c
        if c.test == "count_walk_trunc":
            p = int(c.name.split("<")[1].split(",")[0])
            assert p == max(10, ss.planes_for(ss.BATCH_MAX_POS[c.batch])), c


def test_refine_units_pair_with_fourteen_planes():
    """search_plan.hpp check_refine_units: 14-plane refine units go with an emit kernel of 14 planes or more, never another."""
    for name in ss.printable_names():
        for fam, a in ss.launched(name):
            if fam == "count_refine_emit_kernel" and a[1] == 14:
                assert a[0] >= 14, name
