"""The masked-search addition to the C ABI (include/codd_knn.h): the built library exports the call, native.py
binds it with the header's signature, the header declares it with its options and stats, and what it answers without a device.
No GPU."""

import ctypes
import os
import re

from codd_query_engine_amd import native
from codd_query_engine_amd.knn_index import DeviceKnnIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "codd_knn_search_masked"


def test_the_library_exports_the_call_and_native_binds_it():
    lib = native.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in native.ABI}
    assert NAME in bound
    fn = getattr(lib, NAME)                           # AttributeError: the built library does not export it
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(bound[NAME][1])
    assert bound[NAME][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def test_the_header_declares_what_native_binds():
    header = open(os.path.join(ROOT, "include", "codd_knn.h")).read()
    declared = set(re.findall(r"\b(codd_knn_\w+)\s*\(", header))
    assert {name for name, _, _ in native.ABI} <= declared
    flat = re.sub(r"\s+", " ", header)
    assert ("int codd_knn_search_masked(codd_knn_index* index, const float* dev_queries, int B, int k, const uint32_t* host_allow_bits, "
            "int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);") in flat
    for word in ('"mask_route"', '"mask_list_pct"', '"masked_searches"', '"mask_list_searches"', '"mask_dense_searches"', '"last_mask_rows"'):
        assert word in header, word
    assert "_search_masked" in header.split("#ifndef CODD_KNN_H")[0], "listed among the thread-safe search entry points"


def test_null_arguments_are_einval_not_a_crash():
    lib = native.load()
    words = (ctypes.c_uint32 * 2)(0xFFFFFFFF, 1)
    assert lib.codd_knn_search_masked(None, None, 1, 1, words, 2, 0, None, None, None, None) == -22
    assert b"null" in lib.codd_knn_last_error()


def test_the_python_owner_has_the_three_methods():
    for name in ("search_masked", "search_masked_tensors", "search_keys_masked"):
        assert callable(getattr(DeviceKnnIndex, name))
