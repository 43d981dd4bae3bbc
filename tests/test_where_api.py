"""`where=` on the device, the parts that need no GPU: the header names the new entry points, limits and stats and
agrees with the Python side's numbers; the program struct has the header's layout; the library's host validation answers without
a device; and the opt-in changes nothing on an engine without eval_where — with it or without it the façade on the checker engine
makes the same calls and gives the same answers."""

import ctypes
import os
import re

import numpy as np
import pytest

from codd_query_engine_amd import native
from codd_query_engine_amd import where_columns as wc
from tests import _where_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codd_knn.h"), encoding="utf-8").read()


def defined(name: str) -> int:
    m = re.search(r"^#define\s+" + name + r"\s+(\S+)", HEADER, re.M)
    assert m, name
    return int(m.group(1), 0)


def test_the_header_names_the_entry_points_and_the_stats():
    for name in ("codd_knn_set_column_host", "codd_knn_drop_columns", "codd_knn_eval_where"):
        assert re.search(r"^int " + name + r"\(", HEADER, re.M), name
        assert name in [n for n, _, _ in native.ABI]
    for stat in ('"where_evals"', '"where_columns"', '"where_column_bytes"', '"where_max_blocks"'):
        assert stat in HEADER, stat


def test_the_limits_agree_everywhere():
    assert defined("CODD_KNN_MAX_COLUMNS") == wc.MAX_COLUMNS == native.MAX_COLUMNS == 32
    assert defined("CODD_KNN_WHERE_MAX_LEAVES") == wc.MAX_LEAVES == native.WHERE_MAX_LEAVES == 32
    assert defined("CODD_KNN_WHERE_MAX_LITERALS") == wc.MAX_LITERALS == native.WHERE_MAX_LITERALS == 256
    assert defined("CODD_KNN_WHERE_MAX_OPS") == wc.MAX_OPS == native.WHERE_MAX_OPS == 64
    assert [defined("CODD_KNN_WHERE_TAG_" + n) for n in ("ABSENT", "BOOL", "NUMBER", "STR")] == [wc.TAG_ABSENT, wc.TAG_BOOL, wc.TAG_NUMBER, wc.TAG_STR]
    assert [defined("CODD_KNN_WHERE_" + n) for n in ("IN", "LT", "LE", "GT", "GE")] == [wc.KIND_IN, wc.KIND_LT, wc.KIND_LE, wc.KIND_GT, wc.KIND_GE]
    assert (defined("CODD_KNN_WHERE_AND"), defined("CODD_KNN_WHERE_OR")) == (wc.OP_AND, wc.OP_OR) and wc.OP_AND >= wc.MAX_LEAVES


def test_the_program_struct_has_the_headers_layout():
    assert ctypes.sizeof(native.WhereLeaf) == 8
    assert ctypes.sizeof(native.WhereProgram) == 16 + 8 * 32 + 64 + 8 * 256 < 4096
    assert native.WhereProgram.leaves.offset == 16 and native.WhereProgram.ops.offset == 272 and native.WhereProgram.literals.offset == 336
    prog = wc.compile_where({"$and": [{"n": {"$gt": 1}}, {"n": {"$in": [2, 3]}}]}, cases.build_columns(type("C", (), {"_metadatas": [{"n": 1}]}), ["n"]).by_key)
    c = native.where_program(prog)
    assert (c.nleaves, c.nliterals, c.nops) == (2, 3, 3) and list(c.ops[:3]) == [0, 1, wc.OP_AND]
    assert (c.leaves[1].column, c.leaves[1].tag, c.leaves[1].kind, c.leaves[1].negate, c.leaves[1].lit_first, c.leaves[1].lit_count) == (0, 2, 0, 0, 1, 2)
    assert list(c.literals[:3]) == [wc.number_key(v) for v in (1, 2, 3)]
    too_long = type("P", (), {"leaves": [(0, 2, 0, 0, 0, 0)] * 33, "literals": [], "ops": [0]})
    with pytest.raises(ValueError):
        native.where_program(too_long)


def test_error_codes_without_a_device():
    lib = native.load()
    assert lib.codd_knn_eval_where(None, None, None, 0, None) == -22
    assert lib.codd_knn_drop_columns(None) == -22
    assert lib.codd_knn_set_column_host(None, 0, None, None, None, 0) == -22
    assert "null" in native.last_error() or "bad" in native.last_error()


# ---------------------------------------------------------------------------------------------- the façade on an engine without eval_where
QUERIES = np.random.default_rng(8).standard_normal((3, cases.DIM)).astype(np.float32)


def answers(col, where, **kw):
    out = col.query(query_embeddings=QUERIES, n_results=7, where=where, **kw)
    return out["ids"], out["distances"]


@pytest.fixture(scope="module")
def twins():
    plain, _, _ = cases.random_collection(500, seed=21, deleted=40)
    by_metadata, _, _ = cases.random_collection(500, seed=21, deleted=40, metadata={"codd:device_where": 1})
    by_client, _, _ = cases.random_collection(500, seed=21, deleted=40, client=cases.host_client(device_where=True))
    assert not plain.device_where and by_metadata.device_where and by_client.device_where
    return plain, by_metadata, by_client


@pytest.mark.parametrize("where", cases.FILTERS[::4] + cases.HOST_FILTERS[:1], ids=lambda w: repr(w)[:60])
def test_the_opt_in_changes_nothing_on_an_engine_without_eval_where(twins, where):
    plain, by_metadata, by_client = twins
    want = answers(plain, where)
    for col in (by_metadata, by_client):
        before = len(col._engine.calls)
        assert answers(col, where) == want
        assert not col._has_device_where() and len(col._columns) == 0 and col._where_bits_cache == {}
        assert set(col._engine.calls[before:]) <= {"search_masked"}, col._engine.calls[before:]


def test_without_the_opt_in_the_calls_are_the_ones_made_before(twins):
    plain = twins[0]
    where = {"$and": [{"size": {"$gt": -2}}, {"color": {"$ne": "red"}}]}
    before = len(plain._engine.calls)
    ids, _ = answers(plain, [where, None, {"namespace": "ns0"}])
    assert plain._engine.calls[before:] == ["search", "search_scoped", "search_masked"]
    mask = plain._engine.masks[-1]
    assert np.array_equal(mask, plain._eval_where(where)) and len(plain._columns) == 0
    assert all(i for i in ids)


def test_writes_on_an_opted_in_collection_without_columns_send_nothing_to_the_engine(twins):
    col = twins[2]
    col.upsert(ids=["extra"], embeddings=QUERIES[:1], metadatas=[{"size": 1}])
    assert not hasattr(col._engine, "set_column") and len(col._columns) == 0
    col.delete(ids=["extra"])
