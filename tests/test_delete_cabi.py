"""The delete / compact additions to the C ABI (include/codd_knn.h): the built library exports the three
calls, native.py binds them with the header's signatures, the header declares them, and what they answer without a device.  No GPU."""

import ctypes
import os
import re

from codd_query_engine_amd import native
from codd_query_engine_amd.knn_index import DeviceKnnIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("codd_knn_delete_host", "codd_knn_live_count", "codd_knn_compact")


def test_the_library_exports_the_three_calls_and_native_binds_them():
    lib = native.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in native.ABI}
    for name in NEW:
        assert name in bound, name
        fn = getattr(lib, name)                       # AttributeError: the built library does not export it
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(bound[name][1])
    assert bound["codd_knn_delete_host"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    assert bound["codd_knn_live_count"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    assert bound["codd_knn_compact"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]


def test_the_header_declares_what_native_binds():
    header = open(os.path.join(ROOT, "include", "codd_knn.h")).read()
    declared = set(re.findall(r"\b(codd_knn_\w+)\s*\(", header))
    assert {name for name, _, _ in native.ABI} <= declared
    assert re.search(r"int codd_knn_delete_host\(codd_knn_index\* index, const int64_t\* host_slots, int64_t n\);", header)
    assert re.search(r"int codd_knn_live_count\(const codd_knn_index\* index, int64_t\* out\);", header)
    assert re.search(r"int codd_knn_compact\(codd_knn_index\* index, int64_t\* new_count\);", header)
    for stat in ('"dead_rows"', '"delete_calls"', '"compactions"'):
        assert stat in header, stat


def test_null_arguments_are_einval_not_a_crash():
    lib = native.load()
    out = ctypes.c_int64(-7)
    slots = (ctypes.c_int64 * 2)(0, 1)
    assert lib.codd_knn_delete_host(None, slots, 2) == -22 and b"delete" in lib.codd_knn_last_error()
    assert lib.codd_knn_live_count(None, ctypes.byref(out)) == -22
    assert lib.codd_knn_compact(None, ctypes.byref(out)) == -22
    assert out.value == -7


def test_the_python_owner_has_the_three_methods():
    for name in ("delete", "live_count", "compact"):
        assert callable(getattr(DeviceKnnIndex, name))
