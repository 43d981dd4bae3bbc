"""The embedder additions to the C ABI (include/codd_knn.h): the built library exports the three calls, native.py
binds them with the header's signatures, and every argument rule answers EINVAL before any device is touched — creating and
destroying an embedder needs none.  No GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

from codd_query_engine_amd import native
from codd_query_engine_amd.embedding import HashingEmbeddingFunction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
WANT = {
    "codd_knn_embedder_create": [ctypes.POINTER(V), I, I, F],
    "codd_knn_embedder_destroy": [V],
    "codd_knn_embed_texts_host": [V, V, V, I64, V, V],
}
DECLARATIONS = [
    "typedef struct codd_knn_embedder codd_knn_embedder;",
    "int codd_knn_embedder_create(codd_knn_embedder** out, int device, int dim, float trigram_weight);",
    "int codd_knn_embedder_destroy(codd_knn_embedder* e);",
    "int codd_knn_embed_texts_host(codd_knn_embedder* e, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n, float* dev_out, "
    "void* stream);",
]
EINVAL = -22
OUT = ctypes.c_void_p(0x1000)   # a non-null "device" address: no call below gets as far as using it


@pytest.fixture()
def embedder():
    lib = native.load()
    h = V()
    assert lib.codd_knn_embedder_create(ctypes.byref(h), 0, 384, 0.35) == 0 and h.value
    yield h
    assert lib.codd_knn_embedder_destroy(h) == 0


def offsets(*values):
    return np.asarray(values, dtype=np.int64)


def test_the_library_exports_the_calls_and_native_binds_them():
    lib = native.load()
    bound = {name: (restype, argtypes) for name, restype, argtypes in native.ABI}
    for name, argtypes in WANT.items():
        assert name in bound, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(bound[name][1]) == argtypes, name


def test_the_header_declares_them_with_their_contract():
    header = open(os.path.join(ROOT, "include", "codd_knn.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for line in DECLARATIONS:
        assert line in flat, line
    assert "#define CODD_KNN_MAX_EMBED_BYTES (1ll << 28)" in header and native.MAX_EMBED_BYTES == 1 << 28 <= 1 << 30
    assert "#define CODD_KNN_MAX_EMBED_TEXTS (1ll << 24)" in header and native.MAX_EMBED_TEXTS == 1 << 24
    for word in ("store.py:314-316", "store.py:236-238", "HashingEmbeddingFunction", "consumed before the call returns", "0x80"):
        assert word in header, word


def test_create_checks_its_arguments_and_touches_no_device():
    lib = native.load()
    h = V()
    for dim in (7, 0, -1, 4097):
        assert lib.codd_knn_embedder_create(ctypes.byref(h), 0, dim, 0.35) == EINVAL and not h.value, dim
        assert "dim" in native.last_error()
    for tw in (float("nan"), float("inf"), float("-inf"), 1e39):   # (1e39 is infinite as fp32)
        assert lib.codd_knn_embedder_create(ctypes.byref(h), 0, 384, tw) == EINVAL and not h.value, tw
        assert "finite" in native.last_error()
    assert lib.codd_knn_embedder_create(ctypes.byref(h), -1, 384, 0.35) == EINVAL
    assert lib.codd_knn_embedder_create(None, 0, 384, 0.35) == EINVAL
    before = native.live_allocations()
    for dim in (8, 4096):
        assert lib.codd_knn_embedder_create(ctypes.byref(h), 0, dim, 0.0) == 0 and h.value
        assert lib.codd_knn_embedder_destroy(h) == 0
    assert native.live_allocations() == before


def test_destroy_of_null_is_ok():
    assert native.load().codd_knn_embedder_destroy(None) == 0


def test_embed_refuses_bad_arguments_before_any_device_use(embedder):
    lib = native.load()
    two = offsets(0, 2, 4)
    call = lambda e, b, o, n, out: lib.codd_knn_embed_texts_host(e, b, None if o is None else o.ctypes.data, n, out, None)  # noqa: E731
    assert call(None, b"abcd", two, 2, OUT) == EINVAL and "null" in native.last_error()
    assert call(embedder, b"abcd", None, 2, OUT) == EINVAL and "null" in native.last_error()
    assert call(embedder, b"abcd", two, -1, OUT) == EINVAL
    assert call(embedder, b"abcd", two, native.MAX_EMBED_TEXTS + 1, OUT) == EINVAL and "MAX_EMBED_TEXTS" in native.last_error()
    assert call(embedder, b"abcd", offsets(1, 2, 4), 2, OUT) == EINVAL and "start at 0" in native.last_error()
    assert call(embedder, b"abcd", offsets(0, 3, 2), 2, OUT) == EINVAL and "non-decreasing" in native.last_error()
    assert call(embedder, b"abcd", offsets(0, -1, 2), 2, OUT) == EINVAL and "non-decreasing" in native.last_error()
    assert call(embedder, b"abcd", offsets(0, 2, native.MAX_EMBED_BYTES + 1), 2, OUT) == EINVAL and "MAX_EMBED_BYTES" in native.last_error()
    assert call(embedder, None, two, 2, OUT) == EINVAL and "null bytes" in native.last_error()
    assert call(embedder, b"ab\x80d", two, 2, OUT) == EINVAL and "0x80" in native.last_error()
    assert call(embedder, b"abc\xff", two, 2, OUT) == EINVAL and "0x80" in native.last_error()
    assert call(embedder, b"abcd", two, 2, None) == EINVAL and "null output" in native.last_error()


def test_no_text_is_ok_and_launches_nothing(embedder):
    lib = native.load()
    zero = offsets(0)
    before = native.live_allocations()
    assert lib.codd_knn_embed_texts_host(embedder, None, zero.ctypes.data, 0, None, None) == 0
    assert lib.codd_knn_embed_texts_host(embedder, b"", zero.ctypes.data, 0, OUT, None) == 0
    assert native.live_allocations() == before, "nothing was staged"


def test_the_python_embedder_checks_the_width_and_closes_cleanly():
    e = HashingEmbeddingFunction(8192)
    with pytest.raises(ValueError, match="4096"):
        e.embed_on_device(["a"], "cuda:0")
    assert e(["a"]).shape == (1, 8192)          # (__call__ has no such limit)
    e.close()
    e.close()
