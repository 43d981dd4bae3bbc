"""codd_knn_debug_last_pass (include/codd_knn.h): declared, exported, bound; the argument errors that need no device; the struct
the binding reads has the header's fields in the header's order.  (EINVAL for a workspace no filter pass has run on needs an index,
hence a device: tests/test_gpu_filter_stages.py::test_read_back_without_a_pass_is_an_argument_error.)"""

import ctypes
import os
import re

from codd_query_engine_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codd_knn.h")).read()


def test_entry_point_is_declared_exported_and_bound():
    assert re.search(r"\bint\s+codd_knn_debug_last_pass\s*\(", HEADER)
    assert hasattr(native.load(), "codd_knn_debug_last_pass")
    assert "codd_knn_debug_last_pass" in [n for n, _, _ in native.ABI]


def test_null_index_is_an_argument_error_and_nothing_is_written():
    lib = native.load()
    info = native.LastPassInfo()
    ctypes.memset(ctypes.byref(info), 0x5A, ctypes.sizeof(info))
    buf = (ctypes.c_uint64 * 1024)(*([0x5A5A5A5A5A5A5A5A] * 1024))
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.codd_knn_debug_last_pass(None, None, ctypes.byref(info), p, p, p, p, p, 4, p, 1024, p, 8) == -22
    assert "null index" in native.last_error()
    assert lib.codd_knn_debug_last_pass(None, None, None, None, None, None, None, None, 0, None, 0, None, 0) == -22
    for sizes in ((-1, 1024, 8), (4, -1, 8), (4, 1024, -1)):     # a negative size, whatever else is passed
        assert lib.codd_knn_debug_last_pass(None, None, ctypes.byref(info), p, p, p, p, p, sizes[0], p, sizes[1], p, sizes[2]) == -22
        assert "negative" in native.last_error()
    assert bytes(info) == b"\x5a" * ctypes.sizeof(info)
    assert all(v == 0x5A5A5A5A5A5A5A5A for v in buf)


def test_struct_matches_the_header():
    body = re.search(r"typedef struct codd_knn_last_pass \{(.*?)\} codd_knn_last_pass;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    declared = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        typ, names = stmt.split(None, 1)
        for name in (x.strip() for x in names.split(",")):
            m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            declared.append((m.group(1), ctype[typ] * int(m.group(2))) if m else (name, ctype[typ]))
    assert [(n, t) for n, t in native.LastPassInfo._fields_] == declared
    assert ctypes.sizeof(native.LastPassInfo) == 96
