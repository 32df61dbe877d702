"""The C ABI of the overlap matrix without a device: libkwage_amd.so exports kwage_group_column_overlaps,
kwage_group_column_overlaps_device and kwage_group_overlap_kernel, kwage_amd/native.py binds them with the header's
argument lists and mirrors kwage_overlap_stats field for field -- the size and the offsets are a C compiler's, from a small
program built against the header --, Group.column_overlaps, Group.column_overlaps_host and FileDatabase.sample_overlaps
have the documented signatures, and both calls make every refusal that needs no look into a group before they touch a GPU,
with their outputs untouched."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from kwage_amd import native

NAMES = ("kwage_group_column_overlaps_device", "kwage_group_column_overlaps")
FIELDS = ("n_a", "n_b", "rows", "tiles", "splits", "straight_blocks", "gathered_blocks", "symmetric", "kernel_ms")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(native.lib_path()):
        native.build_native()
    return native.lib()


def test_the_library_exports_the_symbols(L):
    for name in NAMES + ("kwage_group_overlap_kernel",):
        assert hasattr(C.CDLL(native.lib_path()), name), "libkwage_amd.so does not export %s" % name
    assert L.kwage_abi_version() == 1          # additions only
    assert L.kwage_group_overlap_kernel() in (b"", None) or isinstance(L.kwage_group_overlap_kernel(), bytes)


def test_native_declares_them_as_the_header_does():
    header = open(os.path.join(ROOT, "include", "kwage_amd.h")).read()
    sig = {name: (res, args) for name, res, args in native._SIGNATURES}
    ctype = {"kwage_group *": C.c_void_p, "const uint64_t *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "void *": C.c_void_p,
             "uint32_t *": C.c_void_p, "kwage_overlap_stats *": C.POINTER(native.OverlapStats)}
    for name in NAMES:
        assert name in native.EXPORTED_SYMBOLS and name in sig
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in kwage_amd.h" % name
        want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
        res, args = sig[name]
        assert res is C.c_int and list(args) == want, (name, args, want)
    assert re.search(r"const char \*kwage_group_overlap_kernel\(void\);", header) and sig["kwage_group_overlap_kernel"] == (C.c_char_p, [])
    # the struct, member by member in the header's order (several members may share a line)
    field = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    body = re.search(r"typedef struct \{([^}]*)\} kwage_overlap_stats;", header).group(1)
    members = []
    for line in body.splitlines():
        line = re.sub(r"/\*.*?\*/", "", line).strip()
        if line:
            d = re.match(r"(\w+)\s+(.*);$", line)
            members.extend((n.strip(), field[d.group(1)]) for n in d.group(2).split(","))
    assert [(n, t) for n, t in native.OverlapStats._fields_] == members, (native.OverlapStats._fields_, members)
    assert tuple(n for n, _ in members) == FIELDS


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_the_struct_layout_is_the_c_compilers(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"kwage_amd.h\"\nint main(void)\n{\n"
                   "\tprintf(\"%zu\", sizeof(kwage_overlap_stats));\n" +
                   "".join("\tprintf(\" %%zu\", offsetof(kwage_overlap_stats, %s));\n" % f for f in FIELDS) + "\treturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([shutil.which("gcc") or shutil.which("cc"), "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(native.OverlapStats)] + [getattr(native.OverlapStats, f).offset for f in FIELDS], got
    assert got == [64, 0, 8, 16, 24, 32, 40, 48, 56, 60]


def test_the_python_methods():
    from kwage_amd import engine
    p = inspect.signature(engine.Group.column_overlaps).parameters
    assert list(p) == ["self", "cols", "other", "other_cols", "out", "timing"]
    assert all(p[k].default is None for k in ("cols", "other", "other_cols", "out")) and p["timing"].default is False
    p = inspect.signature(engine.Group.column_overlaps_host).parameters
    assert list(p) == ["self", "cols", "other", "other_cols", "timing"]
    p = inspect.signature(engine.FileDatabase.sample_overlaps).parameters
    assert list(p) == ["self", "accessions", "jaccard"] and p["accessions"].default is None and p["jaccard"].default is False


def test_refusals_that_need_no_device(L):
    """The first three kinds of the header's list, in its order: nothing of a group is read before they are made (the
    group pointers here point nowhere), and the outputs stay as they were."""
    cells = (C.c_uint32 * 4)(7, 7, 7, 7)
    st = native.OverlapStats(n_a=7, tiles=7)
    cols = (C.c_uint64 * 2)(0, 1)
    fake = C.c_void_p(0x1000)                  # never dereferenced
    for fn in (L.kwage_group_column_overlaps, L.kwage_group_column_overlaps_device):
        for a, ca, na, b, cb, nb, out, word in (
                (None, None, 3, fake, cols, 0, None, b"NULL a"),             # (everything later is wrong as well)
                (fake, None, 3, fake, cols, 0, None, b"NULL cells"),
                (fake, None, 3, None, cols, 0, cells, b"NULL cols_a with n_a = 3"),
                (fake, cols, 0, None, cols, 0, cells, b"n_a is 0"),
                (fake, cols, 2, None, None, 5, cells, b"NULL cols_b with n_b = 5"),
                (fake, None, 0, fake, cols, 0, cells, b"n_b is 0"),
                (fake, cols, 2, None, cols, 2, cells, b"cols_b without b")):
            assert fn(a, ca, na, b, cb, nb, out, 0, 2, C.byref(st)) == -1, word
            err = L.kwage_last_error()
            assert word in err and b"kwage_group_column_overlaps" in err, (word, err)
    assert list(cells) == [7, 7, 7, 7] and st.n_a == 7 and st.tiles == 7 and st.kernel_ms == 0
