"""Collection's routing between the host embedder and embed_on_device, on a recording fake embedder and a fake
engine that "lives on a device" (torch's CPU stands in for it): which calls embed where, what the engine is handed, and that a
failing device upsert leaves the host lists as they were.  No GPU."""

import numpy as np
import pytest
import torch

from codd_query_engine_amd.embedding import HashingEmbeddingFunction
from codd_query_engine_amd.knn_client import Collection, KnnClient
from tests._masked_oracle_engine import MaskedOracleEngine

DIM = 64
MIN = 4


class HostOnlyEmbedder:
    """A callable and nothing else: the embedder protocol of before."""

    def __init__(self):
        self.inner = HashingEmbeddingFunction(DIM)
        self.dim = DIM
        self.host_calls = []

    def __call__(self, texts):
        self.host_calls.append(len(texts))
        return self.inner(texts)


class RecordingEmbedder(HostOnlyEmbedder):
    def __init__(self):
        super().__init__()
        self.device_calls = []

    def embed_on_device(self, texts, device):
        self.device_calls.append((len(texts), str(device)))
        return torch.from_numpy(self.inner(list(texts))).to(device)


class HostEngine(MaskedOracleEngine):
    """An engine without a device: numpy in, numpy out."""

    def _prep(self, queries):
        self.query_types.append(type(queries).__name__)
        return super()._prep(queries.numpy() if isinstance(queries, torch.Tensor) else queries)

    def __init__(self, dim, dtype="f32"):
        super().__init__(dim, dtype)
        self.query_types = []
        self.writes = []


class DeviceEngine(HostEngine):
    device = torch.device("cpu")
    fail_next_upsert_device = False

    def search_tensors(self, queries, k):   # (its presence is what the routing rule asks for)
        raise AssertionError("the façade calls search / search_scoped / search_masked")

    def upsert(self, slots, vecs, normalize=True):
        self.writes.append(("upsert", len(slots)))
        super().upsert(slots, vecs, normalize)

    def upsert_device(self, first_slot, vecs, normalize=True):
        assert isinstance(vecs, torch.Tensor) and vecs.dtype == torch.float32 and tuple(vecs.shape)[1] == self.dim
        if self.fail_next_upsert_device:
            raise RuntimeError("device upsert failed")
        self.writes.append(("upsert_device", int(first_slot), vecs.shape[0]))
        MaskedOracleEngine.upsert(self, np.arange(first_slot, first_slot + vecs.shape[0]), vecs.numpy(), normalize)


@pytest.fixture(autouse=True)
def threshold(monkeypatch):
    monkeypatch.setattr(Collection, "DEVICE_EMBED_MIN_TEXTS", MIN)


def collection(embedder, engine_class):
    return KnnClient(embedding_function=embedder, engine_factory=lambda dim: engine_class(dim)).get_or_create_collection("c")


def documents(n, start=0):
    return [f"metric number {i} of service {i % 7} latency" for i in range(start, start + n)]


def fill(col, n=12):
    col.upsert(ids=[f"id{i}" for i in range(n)], documents=documents(n), metadatas=[{"namespace": f"ns{i % 3}", "rank": i} for i in range(n)])


def test_the_threshold_is_a_positive_integer():
    assert isinstance(Collection.__dict__["DEVICE_EMBED_MIN_TEXTS"], int) and Collection.__dict__["DEVICE_EMBED_MIN_TEXTS"] >= 1


def test_an_all_new_upsert_at_the_threshold_embeds_on_the_device_and_fixes_the_width():
    e = RecordingEmbedder()
    col = collection(e, DeviceEngine)
    fill(col, 12)
    assert e.device_calls == [(12, "cpu")] and e.host_calls == []
    assert col._engine.dim == DIM and col._engine.writes == [("upsert_device", 0, 12)]
    col.upsert(ids=["x1", "x2", "x3", "x4"], documents=documents(4, 100))
    assert col._engine.writes[-1] == ("upsert_device", 12, 4) and col.count() == 16
    host = collection(HostOnlyEmbedder(), HostEngine)
    fill(host, 12)
    host.upsert(ids=["x1", "x2", "x3", "x4"], documents=documents(4, 100))
    assert np.array_equal(col._engine.read_rows(), host._engine.read_rows())
    assert col.get() == host.get()


def test_the_host_route_below_the_threshold_for_a_rewritten_id_and_for_given_embeddings():
    e = RecordingEmbedder()
    col = collection(e, DeviceEngine)
    col.upsert(ids=["a", "b", "c"], documents=documents(3))                       # below the threshold
    assert e.device_calls == [] and e.host_calls == [3] and col._engine.writes == [("upsert", 3)]
    col.upsert(ids=["d", "e", "f", "a"], documents=documents(4, 10))               # "a" exists: not a contiguous run of new slots
    assert e.device_calls == [] and e.host_calls == [3, 4] and col._engine.writes[-1] == ("upsert", 4)
    col.upsert(ids=["g", "h", "i", "j"], embeddings=np.ones((4, DIM), dtype=np.float32), documents=documents(4, 20))
    assert e.device_calls == [] and e.host_calls == [3, 4] and col._engine.writes[-1] == ("upsert", 4)
    col.upsert(ids=["k", "l", "m", "n"], documents=documents(4, 30))               # all new, at the threshold
    assert e.device_calls == [(4, "cpu")] and col._engine.writes[-1] == ("upsert_device", 10, 4)


def test_the_host_route_for_an_engine_without_a_device_and_an_embedder_without_embed_on_device():
    e = RecordingEmbedder()
    col = collection(e, HostEngine)
    fill(col)
    col.query(query_texts=documents(6), n_results=3)
    assert e.device_calls == [] and e.host_calls == [12, 6] and set(col._engine.query_types) == {"ndarray"}
    plain = HostOnlyEmbedder()
    col = collection(plain, DeviceEngine)
    fill(col)
    col.query(query_texts=documents(6), n_results=3)
    assert plain.host_calls == [12, 6] and col._engine.writes == [("upsert", 12)] and set(col._engine.query_types) == {"ndarray"}


def test_queries_at_the_threshold_stay_a_device_tensor_on_every_search_path():
    e = RecordingEmbedder()
    col = collection(e, DeviceEngine)
    fill(col)
    host = collection(HostOnlyEmbedder(), HostEngine)
    fill(host)
    texts = documents(6, 3)
    wheres = [None, {"namespace": "ns1"}, {"rank": {"$gte": 5}}, [None, {"namespace": "ns0"}, {"rank": {"$lt": 9}}, {"rank": {"$lt": 9}}, {"namespace": "nobody"}, None]]
    for where in wheres:
        for where_document in (None, {"$contains": "service 3"}):
            if where_document is not None and isinstance(where, list):
                continue
            del col._engine.query_types[:]
            before = len(e.device_calls)
            got = col.query(query_texts=texts, n_results=4, where=where, where_document=where_document)
            assert got == host.query(query_texts=texts, n_results=4, where=where, where_document=where_document), (where, where_document)
            assert e.device_calls[before:] == [(6, "cpu")] and e.host_calls == []
            assert col._engine.query_types and set(col._engine.query_types) == {"Tensor"}, (where, col._engine.query_types)
    del col._engine.query_types[:]
    col.query(query_texts=texts[:3], n_results=4)                                  # below the threshold
    assert e.host_calls == [3] and set(col._engine.query_types) == {"ndarray"}
    col.query(query_texts="one text", n_results=2)
    assert e.host_calls == [3, 1]


def test_a_query_of_the_wrong_width_is_refused_on_the_device_route_too():
    e = RecordingEmbedder()
    col = collection(e, DeviceEngine)
    col.upsert(ids=["a", "b"], embeddings=np.ones((2, 32), dtype=np.float32))
    with pytest.raises(ValueError, match="dimension"):
        col.query(query_texts=documents(5), n_results=1)


def test_a_failing_device_upsert_leaves_the_host_lists_unchanged():
    e = RecordingEmbedder()
    col = collection(e, DeviceEngine)
    fill(col, 6)
    before = (list(col._ids), list(col._documents), list(col._metadatas), dict(col._slot_of), col._engine.read_rows())
    col._engine.fail_next_upsert_device = True
    with pytest.raises(RuntimeError, match="device upsert failed"):
        col.upsert(ids=["n1", "n2", "n3", "n4"], documents=documents(4, 50), metadatas=[{"namespace": "late"}] * 4)
    assert (col._ids, col._documents, col._metadatas, col._slot_of) == before[:4]
    assert np.array_equal(col._engine.read_rows(), before[4]) and col.count() == 6 and "late" not in col._scope_of_namespace
    col._engine.fail_next_upsert_device = False
    col.upsert(ids=["n1", "n2", "n3", "n4"], documents=documents(4, 50))
    assert col.count() == 10 and col._engine.writes[-1] == ("upsert_device", 6, 4)
