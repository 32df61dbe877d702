"""The live insert's C ABI without a device: libkwage_amd.so exports the four entry points include/kwage_amd.h declares,
kwage_amd/native.py binds them with the header's argument lists, and each refuses a NULL group before it touches a GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from kwage_amd import native

SYMBOLS = ("kwage_group_insert_filters", "kwage_group_insert_filters_device", "kwage_group_insert_bloom_files", "kwage_group_retire_columns")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(native.lib_path()):
        native.build_native()
    return native.lib()


def test_the_library_exports_the_four_symbols(L):
    raw = C.CDLL(native.lib_path())
    for name in SYMBOLS:
        assert hasattr(raw, name), "libkwage_amd.so does not export %s" % name
    assert L.kwage_abi_version() == 1          # additions only


def test_native_declares_them_as_the_header_does():
    header = open(os.path.join(ROOT, "include", "kwage_amd.h")).read()
    sig = {name: (res, args) for name, res, args in native._SIGNATURES}
    ctype = {"kwage_group *": C.c_void_p, "const void *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
             "uint64_t *": C.POINTER(C.c_uint64), "float *": C.POINTER(C.c_float), "const char *const *": C.POINTER(C.c_char_p),
             "const uint64_t *": C.c_void_p}
    for name in SYMBOLS:
        assert name in native.EXPORTED_SYMBOLS and name in sig
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in kwage_amd.h" % name
        want = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            want.append(ctype[re.sub(r"\w+$", "", p).strip()])          # the type: the declaration without the parameter's name
        res, args = sig[name]
        assert res is C.c_int and list(args) == want, (name, args, want)


def test_a_null_group_is_refused_without_a_device(L):
    first, ms = C.c_uint64(77), C.c_float(0)
    buf = (C.c_uint8 * 16)()
    assert L.kwage_group_insert_filters(None, buf, 16, 1, 0, C.byref(first), C.byref(ms)) == -1
    assert b"NULL" in L.kwage_last_error()
    assert L.kwage_group_insert_filters_device(None, buf, 16, 1, 0, C.byref(first), None) == -1
    assert L.kwage_group_insert_bloom_files(None, None, 1, 0, C.byref(first), None) == -1
    assert L.kwage_group_retire_columns(None, None, 0) == -1
    assert first.value == 77
