"""The save's C ABI without a device: libkwage_amd.so exports kwage_group_save_db, kwage_amd/native.py binds it with the
header's argument list and mirrors its two structs field for field, and the call refuses NULL arguments before it touches a
GPU or the output path."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from kwage_amd import native

NAME = "kwage_group_save_db"


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
    ctype = {"kwage_group *": C.c_void_p, "const char *": C.c_char_p, "const kwage_save_column *": C.POINTER(native.SaveColumn),
             "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "kwage_save_stats *": C.POINTER(native.SaveStats)}
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, header)
    assert m, "%s is not declared in kwage_amd.h" % NAME
    want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
    res, args = sig[NAME]
    assert res is C.c_int and list(args) == want, (args, want)
    # the structs, member by member in the header's order
    field = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "float": C.c_float, "const char *": C.c_char_p,
             "const kwage_sample_info *": C.POINTER(native.SampleInfo)}
    for struct, cls in (("kwage_save_column", native.SaveColumn), ("kwage_save_stats", native.SaveStats)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        members = []
        for line in body.splitlines():
            line = re.sub(r"/\*.*?\*/", "", line).strip()
            if line:
                d = re.match(r"(.*?)(\w+);$", line)
                members.append((d.group(2), field[d.group(1).strip()]))
        assert [(n, t) for n, t in cls._fields_] == members, (struct, cls._fields_, members)
    assert C.sizeof(native.SaveColumn) == 32 and C.sizeof(native.SaveStats) == 24


def test_null_arguments_are_refused_without_a_device(L, tmp_path):
    out = str(tmp_path / "never.db")
    cols = (native.SaveColumn * 1)()
    st = native.SaveStats(db_bytes=7)
    assert L.kwage_group_save_db(None, out.encode(), cols, 1, 0, C.byref(st)) == -1
    assert b"kwage_group_save_db" in L.kwage_last_error() and b"NULL" in L.kwage_last_error()
    fake = C.c_void_p(8)                           # never dereferenced: the NULL checks come first
    assert L.kwage_group_save_db(fake, None, cols, 1, 0, C.byref(st)) == -1 and b"NULL" in L.kwage_last_error()
    assert L.kwage_group_save_db(fake, out.encode(), None, 1, 0, C.byref(st)) == -1 and b"NULL" in L.kwage_last_error()
    assert L.kwage_group_save_db(fake, out.encode(), cols, 0, 0, C.byref(st)) == -1 and b"n is 0" in L.kwage_last_error()
    assert st.db_bytes == 7 and not os.path.exists(out) and os.listdir(str(tmp_path)) == []
