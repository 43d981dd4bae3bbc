"""An l2 and an ip collection on the HIP engine, text in through the device embedder: what `query` returns —
ids and the distances, bit for bit — is what the engine's contract gives for the embedded texts (tests/_space_reference.py over the
host embedder's vectors, which are the device embedder's), under a namespace, a general `where`, a `where_document`, after a delete,
and in a fresh client after persist and reload."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient
from codd_query_engine_amd.embedding import HashingEmbeddingFunction
from tests import _space_reference as sr

pytestmark = pytest.mark.gpu

N, DIM, K = 300, 384, 9
WORDS = ["http", "request", "latency", "error", "rate", "cpu", "memory", "usage", "disk", "queue", "depth", "database", "p99", "latência", "größe"]


def text(rng, i):
    return " ".join(WORDS[int(j)] for j in rng.integers(0, len(WORDS), size=int(rng.integers(1, 12)))) + f" #{i % 11}"


class Counting(HashingEmbeddingFunction):
    device_calls = 0

    def embed_on_device(self, texts, device):
        self.device_calls += 1
        return super().embed_on_device(texts, device)


def expect(space, embed, docs, queries, member):
    ref = sr.Reference(space, embed(docs), "f32", embed(queries))
    _, dist, rows = ref.topk(len(queries), K, allow=member)
    return [[f"id{r}" for r in row if r >= 0] for row in rows.tolist()], [[float(x) for x, r in zip(drow, row) if r >= 0] for drow, row in zip(dist, rows.tolist())]


@pytest.mark.parametrize("space", sr.SPACES)
def test_text_in_neighbours_out_under_the_space(space, tmp_path):
    import torch

    assert torch.cuda.is_available()
    rng = np.random.default_rng(3)
    docs = [text(rng, i) for i in range(N)]
    metas = [{"namespace": f"ns{i % 4}", "rank": i} for i in range(N)]
    queries = [text(rng, i) for i in range(12)]
    embed = Counting(DIM)
    client = KnnClient(device="cuda:0", embedding_function=embed, path=str(tmp_path))
    col = client.get_or_create_collection("c", metadata={"hnsw:space": space})
    col.upsert(ids=[f"id{i}" for i in range(N)], documents=docs, metadatas=metas)
    assert embed.device_calls == 1 and col._engine.space == space and col._engine.stat("metric") == {"ip": 1, "l2": 2}[space]
    everyone = np.ones(N, dtype=bool)
    cases = [({}, everyone),
             ({"where": {"namespace": "ns2"}}, np.arange(N) % 4 == 2),
             ({"where": {"rank": {"$gte": 120}}}, np.arange(N) >= 120),
             ({"where_document": {"$contains": "latency"}}, np.array(["latency" in d for d in docs]))]
    for kwargs, member in cases:
        got = col.query(query_texts=queries, n_results=K, **kwargs)
        ids, dist = expect(space, embed, docs, queries, member)
        assert got["ids"] == ids and got["distances"] == dist, (space, kwargs)
    assert embed.device_calls == 1 + len(cases), "the queries were embedded on the device"
    gone = [0, 5, 121, 122, 250]
    col.delete(ids=[f"id{i}" for i in gone])
    live = everyone.copy()
    live[gone] = False
    ids, dist = expect(space, embed, docs, queries, live)
    got = col.query(query_texts=queries, n_results=K)
    assert got["ids"] == ids and got["distances"] == dist
    assert client.persist() == 1
    fresh = KnnClient(device="cuda:0", embedding_function=embed, path=str(tmp_path))
    again = fresh.get_or_create_collection("c")
    assert again.space == space and again._engine.space == space and again.count() == N - len(gone)
    assert again.query(query_texts=queries, n_results=K) == got
    got_ns = again.query(query_texts=queries, n_results=K, where={"namespace": "ns1"})
    ids, dist = expect(space, embed, docs, queries, live & (np.arange(N) % 4 == 1))
    assert got_ns["ids"] == ids and got_ns["distances"] == dist
    col.upsert(ids=["late1", "late2"], documents=["queue depth p99", "disk usage"])
    assert client.persist() == 1 and fresh.reload() == 1 and again._engine.space == space and again.count() == N - len(gone) + 2
    embed.close()
