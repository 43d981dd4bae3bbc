"""ChromaDB's other two spaces at the C ABI and in the bindings, without a GPU: the constants and the two metric
merges exist in the header, the library and native.py, codd_knn_create no longer refuses metrics 1 and 2 for being unknown, and
the Python wrappers refuse a space name that is none of the three before they touch the library."""

import ctypes
import os
import re

import pytest

from codd_query_engine_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codd_knn.h")).read()


def test_the_header_defines_the_three_metrics_and_native_mirrors_them():
    found = dict(re.findall(r"#define\s+CODD_KNN_METRIC_(\w+)\s+(\d+)", HEADER))
    assert found == {"COSINE": "0", "IP": "1", "L2": "2"}
    assert (native.METRIC_COSINE, native.METRIC_IP, native.METRIC_L2) == (0, 1, 2)
    assert native.METRIC_CODES == {"cosine": 0, "ip": 1, "l2": 2}
    assert native.METRIC_NAMES == {0: "cosine", 1: "ip", 2: "l2"}
    assert "only cosine exists on the path" not in HEADER


@pytest.mark.parametrize("name", ["codd_knn_merge_keys_metric", "codd_knn_merge_shards_metric"])
def test_the_metric_merges_are_declared_exported_and_bound(name):
    assert re.search(rf"\bint\s+{name}\s*\(", HEADER)
    assert hasattr(native.load(), name)
    assert name in [n for n, _, _ in native.ABI]


def test_argument_checks_that_need_no_device():
    lib = native.load()
    # a bad argument is refused before the metric is looked at, and an unknown metric before any HIP call
    assert lib.codd_knn_merge_keys_metric(0, None, 1, 1, 1, native.METRIC_L2, None, None, None, None) == -22
    assert lib.codd_knn_merge_shards_metric(0, None, 1, 1, 1, 1, native.METRIC_IP, None, None, None, None) == -22
    keys = (ctypes.c_uint64 * 1)(0)
    assert lib.codd_knn_merge_keys_metric(0, keys, 1, 1, 1, 3, None, None, None, None) == -95
    assert lib.codd_knn_merge_shards_metric(0, keys, 1, 1, 1, 1, 7, None, None, None, None) == -95
    assert "metric" in native.last_error()
    h = ctypes.c_void_p()
    for metric in (native.METRIC_IP, native.METRIC_L2):
        assert lib.codd_knn_create(ctypes.byref(h), 0, 0, 0, metric) == -22      # (dim 0: the same answer as for cosine)
    assert lib.codd_knn_create(ctypes.byref(h), 0, 768, 0, 3) == -95
    assert lib.codd_knn_create(ctypes.byref(h), 0, 768, 0, -1) == -95


def test_create_accepts_ip_and_l2():
    """-95 on the parent commit.  Without a GPU the call gets as far as the device lookup: any answer but ENOTSUP."""
    lib = native.load()
    for metric in (native.METRIC_IP, native.METRIC_L2):
        h = ctypes.c_void_p()
        rc = lib.codd_knn_create(ctypes.byref(h), 0, 768, 0, metric)
        assert rc != -95, native.last_error()
        if rc == 0:
            out = ctypes.c_int64(-1)
            assert lib.codd_knn_get_stat(h, b"metric", ctypes.byref(out)) == 0 and out.value == metric
            assert lib.codd_knn_destroy(h) == 0


def test_space_names_are_checked_in_python():
    assert native.metric_code("l2") == 2 and native.metric_code("ip") == 1 and native.metric_code("cosine") == 0
    with pytest.raises(ValueError):
        native.metric_code("euclidean")
    from codd_query_engine_amd import knn_index

    with pytest.raises(ValueError):
        knn_index.DeviceKnnIndex(8, "f32", "cuda:0", space="manhattan")
    with pytest.raises(ValueError):
        knn_index.merge_keys(None, 1, space="manhattan")
    with pytest.raises(ValueError):
        knn_index.merge_shards(None, 1, 1, space="manhattan")
