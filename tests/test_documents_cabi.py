"""The document additions to the C ABI (include/codd_knn.h): the built library exports the three calls, native.py
binds them with the header's signatures, the header declares them with their stats, and what they answer without a device.
No GPU."""

import ctypes
import os
import re

from codd_query_engine_amd import native
from codd_query_engine_amd.knn_index import DeviceKnnIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I, I64, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
WANT = {
    "codd_knn_set_documents_host": [V, V, V, I64],
    "codd_knn_match_documents": [V, V, I, V, I64, V],
    "codd_knn_search_masked_dev": [V, V, I, I, V, I64, U32, V, V, V, V],
}
DECLARATIONS = [
    "int codd_knn_set_documents_host(codd_knn_index* index, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n);",
    "int codd_knn_match_documents(codd_knn_index* index, const uint8_t* host_needle, int needle_len, uint32_t* dev_bits, int64_t nwords, "
    "void* stream);",
    "int codd_knn_search_masked_dev(codd_knn_index* index, const float* dev_queries, int B, int k, const uint32_t* dev_allow_bits, "
    "int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);",
]


def test_the_library_exports_the_calls_and_native_binds_them():
    lib = native.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in native.ABI}
    for name, argtypes in WANT.items():
        assert name in bound, name
        fn = getattr(lib, name)                       # AttributeError: the built library does not export it
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(bound[name][1]) == argtypes, name


def test_the_header_declares_what_native_binds():
    header = open(os.path.join(ROOT, "include", "codd_knn.h")).read()
    declared = set(re.findall(r"\b(codd_knn_\w+)\s*\(", header))
    assert {name for name, _, _ in native.ABI} <= declared
    flat = re.sub(r"\s+", " ", header)
    for line in DECLARATIONS:
        assert line in flat, line
    assert "#define CODD_KNN_MAX_NEEDLE 256" in header and native.MAX_NEEDLE == 256
    for word in ('"docs_valid"', '"doc_bytes"', '"doc_tile_bytes"', '"doc_matches"', '"masked_dev_searches"'):
        assert word in header, word
    conventions = header.split("#ifndef CODD_KNN_H")[0]
    assert "_search_masked_dev" in conventions and "_match_documents" in conventions, "listed among the thread-safe entry points"
    assert "SYNCHRONISES" in header, "the header says that search_masked_dev reads m back"


def test_null_arguments_are_einval_not_a_crash():
    lib = native.load()
    words = (ctypes.c_uint32 * 2)(0xFFFFFFFF, 1)
    offsets = (ctypes.c_int64 * 2)(0, 1)
    assert lib.codd_knn_search_masked_dev(None, None, 1, 1, words, 2, 0, None, None, None, None) == -22
    assert b"null" in lib.codd_knn_last_error()
    assert lib.codd_knn_set_documents_host(None, b"a", offsets, 1) == -22
    assert b"null" in lib.codd_knn_last_error()
    assert lib.codd_knn_match_documents(None, b"a", 1, words, 2, None) == -22
    assert b"null" in lib.codd_knn_last_error()


def test_the_python_owner_has_the_methods():
    for name in ("set_documents", "match_documents", "search_masked_dev", "search_masked_dev_tensors", "search_keys_masked_dev"):
        assert callable(getattr(DeviceKnnIndex, name))
