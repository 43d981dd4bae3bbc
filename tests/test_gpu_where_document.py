"""`where_document` through KnnClient on the device: the scenarios of tests/test_where_document_facade.py with the
needles matched by doc_match_kernel and the search under a mask that never leaves the GPU.  Expected ids and distances are that
file's: `needle in doc` over its documents and the oracle on the rows that pass, bit for bit."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore
from tests.test_where_document_facade import DIM, FILTERS, N, document_of, expected, fill, metadata_of, passes
from tests.test_where_facade import passes as md_passes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def filled():
    import torch

    assert torch.cuda.is_available()
    col = KnnClient(device="cuda:0").get_or_create_collection("docs")
    vecs = fill(col)
    return col, vecs, [document_of(i) for i in range(N)]


@pytest.mark.parametrize("wd", FILTERS, ids=[str(i) for i in range(len(FILTERS))])
def test_query_on_the_device_path(filled, wd):
    col, vecs, docs = filled
    engine = col._engine
    before = (engine.stat("masked_dev_searches"), engine.stat("masked_searches"))
    q = np.random.default_rng(2).standard_normal((3, DIM)).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=7, where_document=wd)
    for b in range(3):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 7)
        assert out["ids"][b] == ids
        assert out["distances"][b] == dist
    assert (engine.stat("masked_dev_searches"), engine.stat("masked_searches")) == (before[0] + 1, before[1] + 1), "one search_masked_dev, nothing else"
    assert engine.stat("docs_valid") == 1 and col._docs_on_device


def test_needle_bitmaps_are_cached_and_the_snapshot_is_uploaded_once(filled):
    col, _, _ = filled
    engine = col._engine
    q = np.ones((1, DIM), dtype=np.float32)
    col.query(query_embeddings=q, where_document={"$contains": "cached needle"})
    matches = engine.stat("doc_matches")
    col.query(query_embeddings=q, where_document={"$or": [{"$contains": "cached needle"}, {"$not_contains": "cached needle"}]})
    assert engine.stat("doc_matches") == matches
    col.query(query_embeddings=q, where_document={"$contains": "another needle"})
    assert engine.stat("doc_matches") == matches + 1
    assert len(col._doc_bits_cache) <= 32


def test_a_cached_needle_costs_no_pass_over_the_documents(filled):
    """With the snapshot on the device and the needle's bitmap cached, a query does not walk the host's documents again (the NUL
    check is made once per change of the collection): the list is swapped for one that counts its iterations."""
    col, vecs, docs = filled

    class Counting(list):
        walks = 0

        def __iter__(self):
            Counting.walks += 1
            return super().__iter__()

    q = np.random.default_rng(12).standard_normal((2, DIM)).astype(np.float32)
    wd = {"$contains": "queue"}
    col.query(query_embeddings=q, n_results=5, where_document=wd)
    assert col._docs_fit_device is True and col._docs_on_device
    plain = col._documents
    col._documents = Counting(plain)
    try:
        matches = col._engine.stat("doc_matches")
        out = col.query(query_embeddings=q, n_results=5, where_document=wd, include=("distances",))
        assert Counting.walks == 0 and col._engine.stat("doc_matches") == matches
    finally:
        col._documents = plain
    for b in range(2):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 5)
        assert out["ids"][b] == ids and out["distances"][b] == dist


@pytest.mark.parametrize("where", [{"namespace": "prod:api"}, {"kind": "gauge"}, {"$and": [{"namespace": "prod:billing"}, {"rank": {"$lt": 40}}]},
                                   {"namespace": "nobody"}])
def test_where_and_where_document_must_both_hold(filled, where):
    col, vecs, docs = filled
    q = np.random.default_rng(4).standard_normal((2, DIM)).astype(np.float32)
    wd = {"$contains": "e"}
    out = col.query(query_embeddings=q, n_results=6, where=where, where_document=wd)
    for b in range(2):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 6, also=lambda i: md_passes(metadata_of(i), where))
        assert out["ids"][b] == ids and out["distances"][b] == dist


def test_the_device_path_and_the_host_path_agree(filled):
    """A needle above CODD_KNN_MAX_NEEDLE bytes is evaluated on the host and uploaded as a mask: the same answer as the kernel's for
    a filter that means the same."""
    col, vecs, docs = filled
    engine = col._engine
    q = np.random.default_rng(8).standard_normal((4, DIM)).astype(np.float32)
    long_needle = "x" * 300                                    # above the cap, in no document
    on_device = col.query(query_embeddings=q, n_results=9, where_document={"$contains": "latency"})
    matches = engine.stat("doc_matches")
    on_host = col.query(query_embeddings=q, n_results=9, where_document={"$and": [{"$contains": "latency"}, {"$not_contains": long_needle}]})
    assert engine.stat("doc_matches") == matches, "the long needle never reaches the kernel"
    assert on_host["ids"] == on_device["ids"] and on_host["distances"] == on_device["distances"]
    assert col.query(query_embeddings=q, n_results=9, where_document={"$contains": long_needle})["ids"] == [[], [], [], []]
    # a long needle that does occur: a document made of one, in a collection of its own
    small = KnnClient(device="cuda:0").get_or_create_collection("long")
    text = "abc" * 120
    small.upsert(ids=["a", "b", "c"], embeddings=np.eye(3, DIM, dtype=np.float32), documents=["zz" + text, text[:-1], None])
    hit = small.query(query_embeddings=np.ones((1, DIM), dtype=np.float32), n_results=3, where_document={"$contains": text})
    assert hit["ids"] == [["a"]]
    assert small._engine.stat("doc_matches") == 0
    hit = small.query(query_embeddings=np.ones((1, DIM), dtype=np.float32), n_results=3, where_document={"$contains": text[:256]})
    assert sorted(hit["ids"][0]) == ["a", "b"] and small._engine.stat("doc_matches") == 1


def test_get_and_the_pass_through_from_the_store(filled):
    col, _, docs = filled
    wd = {"$or": [{"$contains": "queue"}, {"$contains": "latency"}]}
    assert col.get(where_document=wd)["ids"] == [f"id{i}" for i in range(N) if passes(docs[i], wd)]
    store = MetricsSemanticMetadataStore(KnnClient(device="cuda:0"), collection_name="metrics")
    store.index_metadata("prod:api", {"metric_name": "http.latency", "description": "HTTP request latency in milliseconds"})
    store.index_metadata("prod:api", {"metric_name": "http.errors", "description": "HTTP 5xx responses", "category": "errors"})
    store.index_metadata("prod:db", {"metric_name": "db.query.time", "description": "Database query latency", "category": "database"})
    client = MetricsSearchClient(store)
    assert [h["metric_name"] for h in client.search_relevant_metrics("latency", limit=5, where_document={"$contains": "milliseconds"})] == ["http.latency"]
    many = client.search_relevant_metrics_batch(["latency", "errors"], limit=5, namespace=["prod:api", "prod:db"], where_document={"$contains": "latency"})
    assert [[h["metric_name"] for h in r] for r in many] == [["http.latency"], ["db.query.time"]]
    assert store.collection._engine.stat("masked_dev_searches") >= 3


def test_upsert_delete_and_compact_refresh_the_snapshot():
    """Last: its own collection.  Each change drops the snapshot flag and the bitmaps; the next call uploads again and answers right."""
    col = KnnClient(device="cuda:0").get_or_create_collection("churn")
    vecs = fill(col, n=30)
    docs = [document_of(i) for i in range(30)]
    wd = {"$contains": "latency"}
    q = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)

    def check(order):
        out = col.query(query_embeddings=q[None, :], n_results=5, where_document=wd)
        ids, dist = expected(vecs, docs, order, q, wd, 5)
        assert out["ids"][0] == ids and out["distances"][0] == dist
        assert col._docs_on_device and col._engine.stat("docs_valid") == 1

    check(range(30))
    docs[0], docs[1] = "nothing to see", "latency at last"
    col.upsert(ids=["id0", "id1"], embeddings=vecs[[0, 1]], documents=[docs[0], docs[1]])
    assert not col._docs_on_device and not col._doc_bits_cache and col._engine.stat("docs_valid") == 0
    check(range(30))
    col.delete(ids=["id9", "id18"])
    assert not col._doc_bits_cache
    live = [i for i in range(30) if i not in (9, 18)]
    check(live)
    col.compact()
    check(live)
