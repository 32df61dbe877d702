"""The compaction's C ABI without a device: libkwage_amd.so exports kwage_group_compact, kwage_amd/native.py binds it with
the header's argument list and mirrors its stats struct field for field, and the call refuses a NULL group before it touches
a GPU, with its outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from kwage_amd import native

NAME = "kwage_group_compact"


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(native.lib_path()):
        native.build_native()
    return native.lib()


def test_the_library_exports_the_symbol(L):
    assert hasattr(C.CDLL(native.lib_path()), NAME), "libkwage_amd.so does not export %s" % NAME
    assert L.kwage_abi_version() == 1          # additions only


def test_native_declares_it_as_the_header_does():
    header = open(os.path.join(ROOT, "include", "kwage_amd.h")).read()
    sig = {name: (res, args) for name, res, args in native._SIGNATURES}
    assert NAME in native.EXPORTED_SYMBOLS and NAME in sig
    ctype = {"kwage_group *": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint64_t *": C.POINTER(C.c_uint64),
             "kwage_compact_stats *": C.POINTER(native.CompactStats)}
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, header)
    assert m, "%s is not declared in kwage_amd.h" % NAME
    want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
    res, args = sig[NAME]
    assert res is C.c_int and list(args) == want, (args, want)
    # the struct, member by member in the header's order (several members may share a line)
    field = {"uint64_t": C.c_uint64, "float": C.c_float}
    body = re.search(r"typedef struct \{([^}]*)\} kwage_compact_stats;", header).group(1)
    members = []
    for line in body.splitlines():
        line = re.sub(r"/\*.*?\*/", "", line).strip()
        if line:
            d = re.match(r"(\w+)\s+(.*);$", line)
            members.extend((n.strip(), field[d.group(1)]) for n in d.group(2).split(","))
    assert [(n, t) for n, t in native.CompactStats._fields_] == members, (native.CompactStats._fields_, members)
    assert C.sizeof(native.CompactStats) == 56
    d = re.search(r"#define\s+KWAGE_NO_COLUMN\s+(0x[0-9A-Fa-f]+)ull", header)
    assert d and int(d.group(1), 16) == native.NO_COLUMN == 2**64 - 1
    assert np.array([native.NO_COLUMN], dtype=np.uint64).view(np.int64)[0] == -1      # what Group.compact hands out


def test_a_null_group_is_refused_without_a_device(L):
    new = (C.c_uint64 * 4)(7, 7, 7, 7)
    st = native.CompactStats(span_before=7, columns=7)
    assert L.kwage_group_compact(None, 0, new, 4, C.byref(st)) == -1
    assert b"kwage_group_compact" in L.kwage_last_error() and b"NULL" in L.kwage_last_error()
    assert L.kwage_group_compact(None, 2, None, 0, None) == -1
    assert list(new) == [7, 7, 7, 7] and st.span_before == 7 and st.columns == 7 and st.kernel_ms == 0
