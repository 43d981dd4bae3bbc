"""Text in, neighbours out with the embedding on the device: two collections on the HIP engine hold the same
documents, some of them not ASCII; one embeds through HashingEmbeddingFunction.embed_on_device, the other is held to the host route
by an embedder wrapper that exposes only __call__.  Stored rows, ids and distances must be the same bits on both."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient
from codd_query_engine_amd.embedding import HashingEmbeddingFunction
from codd_query_engine_amd.knn_client import Collection

pytestmark = pytest.mark.gpu

N, DIM = 300, 384
WORDS = ["http", "request", "latency", "error", "rate", "cpu", "memory", "usage", "disk", "queue", "depth", "database", "Query", "p99", "GC_pause",
         "latência", "İ", "größe", "naïve", "メトリック"]


class HostOnly:
    def __init__(self, inner):
        self.inner = inner

    def __call__(self, texts):
        return self.inner(texts)


class Counting(HashingEmbeddingFunction):
    device_calls = 0

    def embed_on_device(self, texts, device):
        self.device_calls += 1
        return super().embed_on_device(texts, device)


def text(rng, i):
    return " ".join(WORDS[int(j)] for j in rng.integers(0, len(WORDS), size=int(rng.integers(1, 14)))) + f" #{i % 11}"


@pytest.fixture(scope="module")
def pair():
    import torch

    assert torch.cuda.is_available()
    assert Collection.DEVICE_EMBED_MIN_TEXTS <= 64, "the batches below are meant to take the device route"
    rng = np.random.default_rng(3)
    docs = [text(rng, i) for i in range(N)]
    docs[5], docs[6] = "", "  ...  "
    assert sum(not d.isascii() for d in docs) > 30 and sum(d.isascii() for d in docs) > 30
    metas = [{"namespace": f"ns{i % 4}", "rank": i} for i in range(N)]
    ids = [f"id{i}" for i in range(N)]
    counting = Counting(DIM)
    on_device = KnnClient(device="cuda:0", embedding_function=counting).get_or_create_collection("device")
    on_host = KnnClient(device="cuda:0", embedding_function=HostOnly(HashingEmbeddingFunction(DIM))).get_or_create_collection("host")
    for col in (on_device, on_host):
        col.upsert(ids=ids[:200], documents=docs[:200], metadatas=metas[:200])
        col.upsert(ids=ids[200:], documents=docs[200:], metadatas=metas[200:])
    assert counting.device_calls == 2
    yield on_device, on_host, counting, rng
    counting.close()


def test_stored_rows_are_bit_equal(pair):
    on_device, on_host, _, _ = pair
    a, b = on_device._engine.read_rows(), on_host._engine.read_rows()
    assert a.shape == b.shape == (N, DIM) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kwargs", [
    {},
    {"where": {"namespace": "ns2"}},
    {"where": {"rank": {"$gte": 120}}},
    {"where_document": {"$contains": "latency"}},
    {"where": {"rank": {"$lt": 250}}, "where_document": {"$not_contains": "cpu"}},
], ids=["plain", "namespace", "where", "where_document", "both"])
def test_queries_give_identical_ids_and_distances(pair, kwargs):
    on_device, on_host, counting, _ = pair
    rng = np.random.default_rng(17)
    queries = [text(rng, i) for i in range(70)]
    assert any(not q.isascii() for q in queries) and any(q.isascii() for q in queries)
    before = counting.device_calls
    got = on_device.query(query_texts=queries, n_results=9, **kwargs)
    want = on_host.query(query_texts=queries, n_results=9, **kwargs)
    assert counting.device_calls == before + 1, "the device route ran"
    assert got["ids"] == want["ids"] and got["distances"] == want["distances"]
    assert got == want and any(len(hits) == 9 for hits in got["ids"])


def test_embed_on_device_is_the_host_embedder_bit_for_bit(pair):
    _, _, counting, _ = pair
    texts = ["", "latência", "plain ascii", "İ", "MiXed Case_9", "ß", "a" * 500, "x\x00y", "tab\tsep"] * 3
    got = counting.embed_on_device(texts, "cuda:0")
    assert got.is_cuda and tuple(got.shape) == (len(texts), DIM)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), counting(texts).view(np.uint32))
    assert tuple(counting.embed_on_device([], "cuda:0").shape) == (0, DIM)
    only_unicode = counting.embed_on_device(["é", "ü"], "cuda:0")
    assert np.array_equal(only_unicode.cpu().numpy().view(np.uint32), counting(["é", "ü"]).view(np.uint32))
