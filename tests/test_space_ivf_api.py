"""IVF on an ip or l2 index at the C ABI, in the bindings and in the façade, without a GPU: the option and the stat
"space_ivf" exist and are documented; ivf.py's space check passes for cosine, and for ip and l2 only with the option on, with the
message that names cosine otherwise; IvfShardEngine reports its index's space; collection metadata {"codd:space_ivf": 1} reaches
the engine's set_option when the engine is created and again after a reload."""

import ctypes
import os

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, ivf, native
from tests import _space_oracle_engine as soe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codd_knn.h")).read()


def test_the_header_documents_the_option():
    assert '"space_ivf"' in HEADER and "DESIGN.md §22" in HEADER
    doc = HEADER[HEADER.index("Coarse-IVF with exact scores"): HEADER.index("int codd_knn_ivf_install")]
    assert "space_ivf" in doc and "RAW" in doc and "own metric" in doc


def test_option_and_stat_exist():
    """The library knows the option by name; where a device exists it also takes 0 / 1, refuses 2 and reads the value back."""
    blob = open(native.LIB_PATH, "rb").read()
    assert b"space_ivf must be 0 or 1" in blob
    lib = native.load()
    assert lib.codd_knn_set_option(None, b"space_ivf", 1) == -22
    for metric in (native.METRIC_COSINE, native.METRIC_IP, native.METRIC_L2):
        h = ctypes.c_void_p()
        if lib.codd_knn_create(ctypes.byref(h), 0, 200, 0, metric) != 0:
            continue
        out = ctypes.c_int64(-1)
        assert lib.codd_knn_get_stat(h, b"space_ivf", ctypes.byref(out)) == 0 and out.value == 0, "off by default"
        assert lib.codd_knn_set_option(h, b"space_ivf", 2) == -22
        assert lib.codd_knn_set_option(h, b"space_ivf", 1) == 0
        assert lib.codd_knn_get_stat(h, b"space_ivf", ctypes.byref(out)) == 0 and out.value == 1
        assert lib.codd_knn_destroy(h) == 0


class StubIndex:
    def __init__(self, space, on=0):
        self.space, self.on = space, on

    def stat(self, key):
        assert key == "space_ivf"
        return self.on

    def count(self):
        return 5


def test_the_space_check_and_the_shard_engine_s_space():
    assert ivf.IvfShardEngine(StubIndex("cosine"), 2).space == "cosine"
    for space in ("l2", "ip"):
        with pytest.raises(native.NativeLibraryError, match="cosine"):
            ivf.IvfShardEngine(StubIndex(space), 2)
        with pytest.raises(native.NativeLibraryError, match="cosine"):
            ivf.build_ivf(StubIndex(space), 2)
        eng = ivf.IvfShardEngine(StubIndex(space, on=1), 3)
        assert eng.space == space and eng.nprobe == 3 and eng.count() == 5


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


def test_metadata_reaches_set_option_on_create_and_after_reload(tmp_path):
    emb = (3.0 * np.random.default_rng(0).standard_normal((20, 16))).astype(np.float32)
    made = []
    client = KnnClient(engine_factory=recording_factory(made), path=str(tmp_path))
    col = client.get_or_create_collection("m", metadata={"hnsw:space": "l2", "codd:space_ivf": 1})
    col.upsert([f"id{i}" for i in range(20)], embeddings=emb)
    assert len(made) == 1 and made[0].space == "l2" and made[0].options == [("space_ivf", 1)]
    assert client.persist() == 1
    made2 = []
    other = KnnClient(engine_factory=recording_factory(made2), path=str(tmp_path))
    assert len(made2) == 1 and made2[0].options == [("space_ivf", 1)]
    col.upsert(["late"], embeddings=emb[:1])
    assert client.persist() == 1 and other.reload() == 1
    assert len(made2) == 2 and made2[1].options == [("space_ivf", 1)], "reload builds a new engine: the option is set again"
    both = client.get_or_create_collection("b", metadata={"hnsw:space": "ip", "codd:space_filter": 1, "codd:space_ivf": 0})
    both.upsert(["a"], embeddings=emb[:1])
    assert made[-1].options == [("space_filter", 1), ("space_ivf", 0)]
