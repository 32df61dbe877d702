"""The export's C ABI without a device: libkwage_amd.so exports the three calls, kwage_amd/native.py binds them with the
header's argument lists, and each refuses a NULL group before it touches a GPU, with its outputs untouched."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from kwage_amd import native

NAMES = ("kwage_group_export_filters", "kwage_group_export_filters_device", "kwage_group_export_bloom_files")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(native.lib_path()):
        native.build_native()
    return native.lib()


def test_the_library_exports_the_symbols(L):
    raw = C.CDLL(native.lib_path())
    for name in NAMES:
        assert hasattr(raw, name), "libkwage_amd.so does not export %s" % name
    assert L.kwage_abi_version() == 1          # additions only


def test_native_declares_them_as_the_header_does():
    header = open(os.path.join(ROOT, "include", "kwage_amd.h")).read()
    sig = {name: (res, args) for name, res, args in native._SIGNATURES}
    ctype = {"kwage_group *": C.c_void_p, "void *": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
             "const uint64_t *": C.POINTER(C.c_uint64), "float *": C.POINTER(C.c_float),
             "const kwage_save_column *": C.POINTER(native.SaveColumn), "const char *const *": C.POINTER(C.c_char_p)}
    for name in NAMES:
        assert name in native.EXPORTED_SYMBOLS and name in sig
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in kwage_amd.h" % name
        want = [ctype[re.sub(r"\w+$", "", " ".join(p.split())).strip()] for p in m.group(1).split(",")]
        res, args = sig[name]
        assert res is C.c_int and list(args) == want, (name, args, want)


def test_a_null_group_is_refused_without_a_device(L, tmp_path):
    cols = (C.c_uint64 * 2)(0, 1)
    out = (C.c_uint8 * 64)(*([0xA5] * 64))
    ms = C.c_float(7.0)
    assert L.kwage_group_export_filters(None, cols, 2, out, 32, 0, 2, C.byref(ms)) == -1
    assert b"kwage_group_export_filters:" in L.kwage_last_error() and b"NULL" in L.kwage_last_error()
    assert L.kwage_group_export_filters_device(None, cols, 2, out, 32, 2, C.byref(ms)) == -1
    assert b"kwage_group_export_filters_device:" in L.kwage_last_error() and b"NULL" in L.kwage_last_error()
    sc = (native.SaveColumn * 1)()
    path = str(tmp_path / "a.bloom").encode()
    paths = (C.c_char_p * 1)(path)
    assert L.kwage_group_export_bloom_files(None, sc, paths, 1, 0, 2, C.byref(ms)) == -1
    assert b"kwage_group_export_bloom_files:" in L.kwage_last_error() and b"NULL" in L.kwage_last_error()
    assert L.kwage_group_export_filters(None, None, 0, None, 0, 0, 0, None) == -1
    assert bytes(out) == b"\xa5" * 64 and ms.value == 7.0 and os.listdir(str(tmp_path)) == []
