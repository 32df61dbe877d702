"""The C ABI of the nearest-neighbour lists without a device: libkwage_amd.so exports kwage_group_column_neighbors,
kwage_group_column_neighbors_device and kwage_group_neighbors_kernel, kwage_amd/native.py binds them with the header's
argument lists and mirrors kwage_neighbor and kwage_neighbors_stats field for field -- sizes and offsets are a C
compiler's, from a small program built against the header --, Group.column_neighbors, Group.column_neighbors_host and
FileDatabase.sample_neighbors have the documented signatures, and both calls make every refusal that needs no look into a
group before they touch a GPU, with their outputs untouched."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from kwage_amd import native

NAMES = ("kwage_group_column_neighbors_device", "kwage_group_column_neighbors")
FIELDS = ("n_a", "n_b", "rows", "strips", "strip_entries", "tiles", "records", "metric", "kernel_ms")
RECORD = ("index", "shared", "bits_a", "bits_b")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(native.lib_path()):
        native.build_native()
    return native.lib()


def test_the_library_exports_the_symbols(L):
    for name in NAMES + ("kwage_group_neighbors_kernel",):
        assert hasattr(C.CDLL(native.lib_path()), name), "libkwage_amd.so does not export %s" % name
    assert L.kwage_abi_version() == 1          # additions only
    assert L.kwage_group_neighbors_kernel() in (b"", None) or isinstance(L.kwage_group_neighbors_kernel(), bytes)


def members_of(header, name):
    """[(member, ctypes type)] of a typedef'd struct of the header, in its order (several members may share a line)."""
    field = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    members = []
    for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace(";", ";\n").splitlines():
        line = line.strip()
        if line:
            d = re.match(r"(\w+)\s+(.*);$", line)
            members.extend((n.strip(), field[d.group(1)]) for n in d.group(2).split(","))
    return members


def test_native_declares_them_as_the_header_does():
    header = open(os.path.join(ROOT, "include", "kwage_amd.h")).read()
    sig = {name: (res, args) for name, res, args in native._SIGNATURES}
    ctype = {"kwage_group *": C.c_void_p, "const uint64_t *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "void *": C.c_void_p,
             "uint32_t *": C.c_void_p, "kwage_neighbor *": C.c_void_p, "kwage_neighbors_stats *": C.POINTER(native.NeighborsStats)}
    for name in NAMES:
        assert name in native.EXPORTED_SYMBOLS and name in sig
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in kwage_amd.h" % name
        want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
        res, args = sig[name]
        assert res is C.c_int and list(args) == want and len(want) == 13, (name, args, want)
    assert re.search(r"const char \*kwage_group_neighbors_kernel\(void\);", header) and sig["kwage_group_neighbors_kernel"] == (C.c_char_p, [])
    assert [(n, t) for n, t in native.NeighborsStats._fields_] == members_of(header, "kwage_neighbors_stats")
    assert tuple(n for n, _ in native.NeighborsStats._fields_) == FIELDS
    assert [(n, t) for n, t in native.Neighbor._fields_] == members_of(header, "kwage_neighbor") == [(n, C.c_uint32) for n in RECORD]
    for macro, value in (("KWAGE_NEIGHBORS_SHARED", "0u"), ("KWAGE_NEIGHBORS_JACCARD", "1u"), ("KWAGE_NEIGHBORS_SKIP_SELF", "0x100u")):
        assert re.search(r"#define %s\s+%s\b" % (macro, value), header), macro


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_the_struct_layouts_are_the_c_compilers(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"kwage_amd.h\"\nint main(void)\n{\n"
                   "\tprintf(\"%zu\", sizeof(kwage_neighbors_stats));\n" +
                   "".join("\tprintf(\" %%zu\", offsetof(kwage_neighbors_stats, %s));\n" % f for f in FIELDS) +
                   "\tprintf(\" %zu\", sizeof(kwage_neighbor));\n" +
                   "".join("\tprintf(\" %%zu\", offsetof(kwage_neighbor, %s));\n" % f for f in RECORD) +
                   "\tprintf(\" %u %u %u %u\", KWAGE_NEIGHBORS_SHARED, KWAGE_NEIGHBORS_JACCARD, KWAGE_NEIGHBORS_SKIP_SELF, KWAGE_TOPK_MAX);\n\treturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([shutil.which("gcc") or shutil.which("cc"), "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:10] == [C.sizeof(native.NeighborsStats)] + [getattr(native.NeighborsStats, f).offset for f in FIELDS], got
    assert got[:10] == [64, 0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert got[10:15] == [C.sizeof(native.Neighbor)] + [getattr(native.Neighbor, f).offset for f in RECORD] == [16, 0, 4, 8, 12]
    assert got[15:] == [0, 1, 0x100, 1024]


def test_the_python_methods():
    from kwage_amd import engine
    for fn in (engine.Group.column_neighbors, engine.Group.column_neighbors_host):
        p = inspect.signature(fn).parameters
        assert list(p) == ["self", "k", "cols", "other", "other_cols", "metric", "min_shared", "skip_self", "timing"]
        assert p["k"].default is inspect.Parameter.empty and all(p[k].default is None for k in ("cols", "other", "other_cols"))
        assert (p["metric"].default, p["min_shared"].default, p["skip_self"].default, p["timing"].default) == ("jaccard", 0, False, False)
    p = inspect.signature(engine.FileDatabase.sample_neighbors).parameters
    assert list(p) == ["self", "k", "accessions", "metric", "min_shared", "skip_self"]
    assert (p["accessions"].default, p["metric"].default, p["min_shared"].default, p["skip_self"].default) == (None, "jaccard", 0, True)


def test_refusals_that_need_no_device(L):
    """The header's list from its start, in its order: nothing of a group is read before these are made (the group
    pointers here point nowhere), and the outputs stay as they were."""
    out = (C.c_uint32 * 8)(*([7] * 8))
    counts = (C.c_uint32 * 2)(7, 7)
    st = native.NeighborsStats(n_a=7, tiles=7, records=7)
    cols = (C.c_uint64 * 2)(0, 1)
    fake = C.c_void_p(0x1000)                  # never dereferenced
    for fn in (L.kwage_group_column_neighbors, L.kwage_group_column_neighbors_device):
        for a, ca, na, b, cb, nb, k, metric, o, c, word in (
                (None, None, 3, fake, cols, 0, 0, 9, None, None, b"NULL a"),            # (everything later is wrong as well)
                (fake, None, 3, fake, cols, 0, 0, 9, None, None, b"NULL out"),
                (fake, None, 3, fake, cols, 0, 0, 9, out, None, b"NULL counts"),
                (fake, None, 3, fake, cols, 0, 0, 9, out, counts, b"k = 0"),
                (fake, None, 3, fake, cols, 0, 1025, 9, out, counts, b"k = 1025"),
                (fake, None, 3, fake, cols, 0, 1024, 2, out, counts, b"unknown metric 2"),
                (fake, None, 3, None, cols, 0, 1, 0, out, counts, b"NULL cols_a with n_a = 3"),
                (fake, cols, 0, None, cols, 0, 1, 1, out, counts, b"n_a is 0"),
                (fake, cols, 2, None, None, 5, 1, 1, out, counts, b"NULL cols_b with n_b = 5"),
                (fake, None, 0, fake, cols, 0, 1, 1, out, counts, b"n_b is 0"),
                (fake, cols, 2, None, cols, 2, 1, 1, out, counts, b"cols_b without b")):
            assert fn(a, ca, na, b, cb, nb, k, metric, 0, o, c, 2 | 0x100, C.byref(st)) == -1, word
            err = L.kwage_last_error()
            assert word in err and b"kwage_group_column_neighbors" in err, (word, err)
    assert list(out) == [7] * 8 and list(counts) == [7, 7] and (st.n_a, st.tiles, st.records, st.kernel_ms) == (7, 7, 7, 0)
