"""The C ABI of the union of columns without a device: libkwage_amd.so exports kwage_group_union_columns,
kwage_amd/native.py binds it with the header's argument list and mirrors kwage_union_stats field for field -- the size and
the offsets are a C compiler's, from a small program built against the header --, Group.union_columns and
FileDatabase.union_samples have the documented signatures, and the call refuses NULL arguments before it touches a GPU,
with its outputs untouched."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from kwage_amd import native

NAME = "kwage_group_union_columns"
FIELDS = ("first_column", "sets", "members", "entries", "first_unit", "units", "bytes_written", "kernel_ms")


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
    ctype = {"kwage_group *": C.c_void_p, "const uint64_t *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
             "uint64_t *": C.POINTER(C.c_uint64), "kwage_union_stats *": C.POINTER(native.UnionStats)}
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, header)
    assert m, "%s is not declared in kwage_amd.h" % NAME
    want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
    res, args = sig[NAME]
    assert res is C.c_int and list(args) == want, (args, want)
    # the struct, member by member in the header's order (several members may share a line)
    field = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    body = re.search(r"typedef struct \{([^}]*)\} kwage_union_stats;", header).group(1)
    members = []
    for line in body.splitlines():
        line = re.sub(r"/\*.*?\*/", "", line).strip()
        if line:
            d = re.match(r"(\w+)\s+(.*);$", line)
            members.extend((n.strip(), field[d.group(1)]) for n in d.group(2).split(","))
    assert [(n, t) for n, t in native.UnionStats._fields_] == members, (native.UnionStats._fields_, members)
    assert tuple(n for n, _ in members) == FIELDS


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_the_struct_layout_is_the_c_compilers(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"kwage_amd.h\"\nint main(void)\n{\n"
                   "\tprintf(\"%zu\", sizeof(kwage_union_stats));\n" +
                   "".join("\tprintf(\" %%zu\", offsetof(kwage_union_stats, %s));\n" % f for f in FIELDS) + "\treturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([shutil.which("gcc") or shutil.which("cc"), "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(native.UnionStats)] + [getattr(native.UnionStats, f).offset for f in FIELDS], got
    assert got == [64, 0, 8, 16, 24, 32, 40, 48, 56]


def test_the_python_methods():
    from kwage_amd import engine
    p = inspect.signature(engine.Group.union_columns).parameters
    assert list(p) == ["self", "sets", "src", "timing"] and p["src"].default is None and p["timing"].default is False
    p = inspect.signature(engine.FileDatabase.union_samples).parameters
    assert list(p) == ["self", "unions", "retire"] and p["retire"].default is False


def test_null_arguments_are_refused_without_a_device(L):
    first = C.c_uint64(0x5A5A)
    st = native.UnionStats(first_column=7, units=7)
    cols = (C.c_uint64 * 2)(0, 1)
    offs = (C.c_uint64 * 2)(0, 2)
    fake = C.c_void_p(0x1000)                  # never dereferenced: the other group is NULL
    for dst, src, word in ((None, None, b"NULL dst"), (None, fake, b"NULL dst"), (fake, None, b"NULL src")):
        assert L.kwage_group_union_columns(dst, src, cols, offs, 1, 0, C.byref(first), C.byref(st)) == -1
        assert NAME.encode() in L.kwage_last_error() and word in L.kwage_last_error()
    assert L.kwage_group_union_columns(None, None, None, None, 0, 2, None, None) == -1
    assert first.value == 0x5A5A and st.first_column == 7 and st.units == 7 and st.kernel_ms == 0
