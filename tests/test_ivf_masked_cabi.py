"""The masked-IVF and mask-slicing additions to the C ABI (include/codd_knn.h): the built library exports the three
calls, native.py binds them with the header's signatures, the header declares them with their stat and names them among the
thread-safe entry points, and what they answer without a device.  No GPU."""

import ctypes
import os
import re

import pytest

from codd_query_engine_amd import ivf, native
from codd_query_engine_amd.knn_index import DeviceKnnIndex
from codd_query_engine_amd.sharded import ShardedSearcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, I64, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
SIGNATURES = {
    "codd_knn_ivf_search_masked": [P, P, I, I, I, P, I64, U32, P, P, P, P],
    "codd_knn_ivf_search_masked_dev": [P, P, I, I, I, P, I64, U32, P, P, P, P],
    "codd_knn_slice_mask": [I, P, I64, I64, I64, P, I64, P],
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_the_library_exports_the_call_and_native_binds_it(name):
    lib = native.load()
    bound = {n: (restype, argtypes) for n, restype, argtypes in native.ABI}
    assert name in bound
    fn = getattr(lib, name)                           # AttributeError: the built library does not export it
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(bound[name][1])
    assert bound[name][1] == SIGNATURES[name]


def test_the_header_declares_what_native_binds():
    header = open(os.path.join(ROOT, "include", "codd_knn.h")).read()
    declared = set(re.findall(r"\b(codd_knn_\w+)\s*\(", header))
    assert {name for name, _, _ in native.ABI} <= declared
    flat = re.sub(r"\s+", " ", header)
    assert ("int codd_knn_ivf_search_masked(codd_knn_index* index, const float* dev_queries, int B, int k, int nprobe, "
            "const uint32_t* host_allow_bits, int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, "
            "void* stream);") in flat
    assert ("int codd_knn_ivf_search_masked_dev(codd_knn_index* index, const float* dev_queries, int B, int k, int nprobe, "
            "const uint32_t* dev_allow_bits, int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, "
            "void* stream);") in flat
    assert ("int codd_knn_slice_mask(int device, const uint32_t* dev_global_bits, int64_t global_rows, int64_t row_base, int64_t count, "
            "uint32_t* dev_out, int64_t nwords, void* stream);") in flat
    assert '"ivf_masked_searches"' in header
    conventions = header.split("#ifndef CODD_KNN_H")[0]
    assert "_ivf_search_masked" in conventions and "_ivf_search_masked_dev" in conventions, "listed among the thread-safe search entry points"


def test_null_arguments_are_einval_not_a_crash():
    lib = native.load()
    words = (ctypes.c_uint32 * 2)(0xFFFFFFFF, 1)
    for fn in (lib.codd_knn_ivf_search_masked, lib.codd_knn_ivf_search_masked_dev):
        assert fn(None, None, 1, 1, 1, words, 2, 0, None, None, None, None) == -22
        assert b"null" in lib.codd_knn_last_error()


def test_slice_mask_checks_its_arguments_before_it_touches_the_device():
    lib = native.load()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused on its arguments
    assert lib.codd_knn_slice_mask(0, fake, -1, 0, 64, fake, 2, None) == -22          # negative global_rows
    assert lib.codd_knn_slice_mask(0, fake, 64, -1, 64, fake, 2, None) == -22         # negative row_base
    assert lib.codd_knn_slice_mask(0, fake, 64, 0, -1, fake, 0, None) == -22          # negative count
    assert lib.codd_knn_slice_mask(0, fake, 64, 0, 64, fake, 3, None) == -22          # nwords != ceil(count / 32)
    assert b"nwords" in lib.codd_knn_last_error()
    assert lib.codd_knn_slice_mask(0, fake, 64, 0, 33, fake, 1, None) == -22
    assert lib.codd_knn_slice_mask(0, None, 64, 0, 64, fake, 2, None) == -22          # global words missing
    assert lib.codd_knn_slice_mask(0, fake, 64, 0, 64, None, 2, None) == -22          # output missing
    assert b"null" in lib.codd_knn_last_error()
    assert lib.codd_knn_slice_mask(0, None, 0, 0, 0, None, 0, None) == 0              # nothing to write: no launch, no device


def test_the_python_layers_have_the_new_surface():
    import inspect

    for name in ("ivf_search_masked_tensors", "ivf_search_keys_masked", "ivf_search_masked_dev_tensors", "ivf_search_keys_masked_dev", "slice_mask"):
        assert callable(getattr(DeviceKnnIndex, name))
    for name in ("search_keys_masked", "search_keys_masked_dev"):
        assert callable(getattr(ivf.IvfShardEngine, name))
    for fn in (ivf.search_ivf, ivf.search_ivf_keys):
        assert inspect.signature(fn).parameters["allow"].default is None
    for name in ("search", "search_async", "search_keys_local"):
        params = inspect.signature(getattr(ShardedSearcher, name)).parameters
        assert params["allow"].default is None and params["allow_global"].default is False
