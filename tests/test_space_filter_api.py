"""The int8 filter leg of an ip or l2 index at the C ABI, in the bindings and in the façade, without a GPU: the
debug entry point codd_knn_filter_slack is declared, exported and bound; the option and the stat "space_filter" exist; collection
metadata {"codd:space_filter": 1} reaches the engine's set_option when the engine is created and again after a reload, and an
engine without set_option still serves such a collection."""

import ctypes
import os
import re

import numpy as np

from codd_query_engine_amd import KnnClient, native
from tests import _space_oracle_engine as soe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codd_knn.h")).read()


def test_filter_slack_is_declared_exported_and_bound():
    assert re.search(r"\bint\s+codd_knn_filter_slack\s*\(", HEADER)
    assert hasattr(native.load(), "codd_knn_filter_slack")
    assert "codd_knn_filter_slack" in [n for n, _, _ in native.ABI]
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert callable(DeviceKnnIndex.filter_slack)
    # argument checks come before any device call
    lib = native.load()
    assert lib.codd_knn_filter_slack(None, None, 1, None, None) == -22
    buf = (ctypes.c_float * 4)()
    assert lib.codd_knn_filter_slack(None, buf, 1, buf, None) == -22


def test_the_header_documents_the_option_and_both_entry_points():
    assert '"space_filter"' in HEADER and "DESIGN.md §21" in HEADER
    doc = HEADER[HEADER.index("The raw approximate (bf16 MFMA) scores"): HEADER.index("int codd_knn_filter_slack")]
    assert "space_filter" in doc and "B <= 32" in doc and "eps(q)" in doc


def test_option_and_stat_exist():
    """The library knows the option by name; where a device exists it also takes 0 / 1, refuses 2 and reads the value back."""
    blob = open(native.LIB_PATH, "rb").read()
    assert b"space_filter must be 0 or 1" in blob
    lib = native.load()
    assert lib.codd_knn_set_option(None, b"space_filter", 1) == -22
    for metric in (native.METRIC_COSINE, native.METRIC_IP, native.METRIC_L2):
        h = ctypes.c_void_p()
        if lib.codd_knn_create(ctypes.byref(h), 0, 200, 0, metric) != 0:
            continue
        out = ctypes.c_int64(-1)
        assert lib.codd_knn_get_stat(h, b"space_filter", ctypes.byref(out)) == 0 and out.value == 0, "off by default"
        assert lib.codd_knn_set_option(h, b"space_filter", 2) == -22
        assert lib.codd_knn_set_option(h, b"space_filter", 1) == 0
        assert lib.codd_knn_get_stat(h, b"space_filter", ctypes.byref(out)) == 0 and out.value == 1
        assert lib.codd_knn_set_option(h, b"space_filter", 0) == 0
        assert lib.codd_knn_destroy(h) == 0


class RecordingEngine(soe.SpaceOracleEngine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.options = []

    def set_option(self, key, value):
        self.options.append((key, value))


def recording_factory(made):
    def make(dim, space="cosine"):
        eng = RecordingEngine(dim, "f32", space)
        made.append(eng)
        return eng

    make.spaces = ("cosine", "l2", "ip")
    return make


def vectors(n, d=16, seed=0):
    return (3.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def test_metadata_reaches_set_option_on_create_and_after_reload(tmp_path):
    made = []
    client = KnnClient(engine_factory=recording_factory(made), path=str(tmp_path))
    col = client.get_or_create_collection("m", metadata={"hnsw:space": "l2", "codd:space_filter": 1})
    emb = vectors(20)
    col.upsert([f"id{i}" for i in range(20)], embeddings=emb)
    assert len(made) == 1 and made[0].space == "l2" and made[0].options == [("space_filter", 1)]
    want = col.query(query_embeddings=emb[:3], n_results=4)
    assert client.persist() == 1

    made2 = []
    other = KnnClient(engine_factory=recording_factory(made2), path=str(tmp_path))        # a second process: loads from disk
    assert len(made2) == 1 and made2[0].options[0] == ("space_filter", 1), "the manifest's metadata switches the leg on"
    got = other.get_collection("m").query(query_embeddings=emb[:3], n_results=4)
    assert got["ids"] == want["ids"] and got["distances"] == want["distances"]

    col.upsert(["late"], embeddings=vectors(1, seed=9))
    assert client.persist() == 1
    assert other.reload() == 1
    assert len(made2) == 2 and ("space_filter", 1) in made2[1].options, "reload builds a new engine: the option is set again"
    assert other.get_collection("m").count() == 21

    # no such key: set_option is not called for it; value 0 is passed on as 0
    plain = client.get_or_create_collection("p", metadata={"hnsw:space": "ip"})
    plain.upsert(["a"], embeddings=vectors(1))
    assert made[-1].space == "ip" and made[-1].options == []
    off = client.get_or_create_collection("o", metadata={"hnsw:space": "ip", "codd:space_filter": 0})
    off.upsert(["a"], embeddings=vectors(1))
    assert made[-1].options == [("space_filter", 0)]


def test_an_engine_without_set_option_still_works():
    made = []
    client = KnnClient(engine_factory=soe.factory("f32", made))
    assert not hasattr(soe.SpaceOracleEngine, "set_option")
    col = client.get_or_create_collection("c", metadata={"hnsw:space": "l2", "codd:space_filter": 1})
    emb = vectors(12, seed=2)
    col.upsert([f"id{i}" for i in range(12)], embeddings=emb)
    res = col.query(query_embeddings=emb[:2], n_results=3)
    assert [r[0] for r in res["ids"]] == ["id0", "id1"] and res["distances"][0][0] == 0.0
