"""`where_document` above the engine, on a checker engine with search_masked only (tests/_masked_oracle_engine.py:
the façade's host path): ChromaDB's document grammar through Collection.query / Collection.get, the store's and
MetricsSearchClient's `where_document=`, the malformed forms, and the caches across upsert / delete / compact.  The expected ids of
every query come from a plain Python `needle in doc` over this file's own documents and the oracle on the rows that pass.  No GPU."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore
from oracle import knn_oracle as o
from tests._masked_oracle_engine import MaskedOracleEngine
from tests._oracle_engine import OracleEngine

DIM = 48
N = 80
NAMESPACES = ["prod:api", "staging:api", "prod:billing"]
WORDS = ["latency", "HTTP", "http", "error", "queue", "Größe", "日本語", "naïve", "rate"]


def masked_client(**kw):
    return KnnClient(engine_factory=lambda dim: MaskedOracleEngine(dim), **kw)


def document_of(i: int):
    """Record i's document: every ninth record has none; the others three of WORDS in the store's own 'a | Label: b' shape."""
    if i % 9 == 8:
        return None
    return f"{WORDS[i % 9]} of service {i} | Unit: {WORDS[(i * 5 + 1) % 9]} | Category: {WORDS[(i * 7 + 3) % 9]}"


def metadata_of(i: int):
    return {"namespace": NAMESPACES[i % 3], "rank": i, "kind": "gauge" if i % 2 else "counter"}


def fill(col, n=N, seed=11):
    vecs = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=[metadata_of(i) for i in range(n)],
               documents=[document_of(i) for i in range(n)])
    return vecs


def passes(doc, wd) -> bool:
    """The filter's meaning, record by record: a record without a document fails $contains and passes $not_contains."""
    (op, arg), = wd.items()
    if op == "$and":
        return all(passes(doc, w) for w in arg)
    if op == "$or":
        return any(passes(doc, w) for w in arg)
    hit = doc is not None and arg in doc
    return hit if op == "$contains" else not hit


def expected(vecs, docs, order, q, wd, k, also=lambda i: True):
    keep = [i for i in order if passes(docs[i], wd) and also(i)]
    if not keep:
        return [], []
    d, i = o.search(o.normalize_rows(vecs[keep]), "f32", o.normalize_rows(q[None, :]), min(k, len(order)))
    hit = i[0] >= 0
    return [f"id{keep[j]}" for j in i[0][hit]], d[0][hit].tolist()


FILTERS = [
    {"$contains": "latency"},
    {"$contains": "http"},                                   # case-sensitive: "HTTP" is another needle
    {"$contains": "HTTP"},
    {"$contains": "Größe"},                                  # multibyte UTF-8
    {"$contains": "日本"},                                    # ... and a prefix of a multibyte word
    {"$contains": "ï"},
    {"$contains": " | Unit: rate"},                          # spans the store's separator
    {"$contains": "service 7"},                              # id7 and the seventies
    {"$not_contains": "error"},                              # records without a document pass
    {"$and": [{"$contains": "http"}, {"$not_contains": "queue"}]},
    {"$or": [{"$contains": "latency"}, {"$contains": "日本語"}]},
    {"$and": [{"$or": [{"$contains": "HTTP"}, {"$contains": "http"}]}, {"$not_contains": "rate"}, {"$contains": "service"}]},
    {"$or": [{"$and": [{"$contains": "error"}, {"$contains": "queue"}]}, {"$not_contains": "e"}]},
    {"$contains": "no such text anywhere"},                  # nobody
]


@pytest.fixture(scope="module")
def filled():
    col = masked_client().get_or_create_collection("docs")
    vecs = fill(col)
    return col, vecs, [document_of(i) for i in range(N)]


@pytest.mark.parametrize("wd", FILTERS, ids=[str(i) for i in range(len(FILTERS))])
def test_query_returns_the_exact_top_k_among_the_documents_that_pass(filled, wd):
    col, vecs, docs = filled
    q = np.random.default_rng(2).standard_normal((3, DIM)).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=7, where_document=wd)
    for b in range(3):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 7)
        assert out["ids"][b] == ids
        assert out["distances"][b] == dist
        assert out["documents"][b] == [docs[int(i[2:])] for i in ids]


def test_nobody_matching_gives_empty_inner_lists_and_fewer_matches_fewer_hits(filled):
    col, vecs, docs = filled
    q = np.random.default_rng(3).standard_normal((2, DIM)).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=5, where_document={"$contains": "no such text anywhere"})
    assert out["ids"] == [[], []] and out["distances"] == [[], []]
    few = col.query(query_embeddings=q, n_results=50, where_document={"$contains": "service 7"})
    want = sum(1 for d in docs if d is not None and "service 7" in d)   # id7 and the seventies that have a document
    assert 1 < want < 50 and all(len(ids) == want for ids in few["ids"])


def test_none_documents_fail_contains_and_pass_not_contains(filled):
    col, _, docs = filled
    none_ids = {f"id{i}" for i in range(N) if docs[i] is None}
    assert none_ids
    assert not none_ids & set(col.get(where_document={"$contains": "e"})["ids"])
    assert none_ids <= set(col.get(where_document={"$not_contains": "e"})["ids"])


def test_matching_is_case_sensitive(filled):
    col, _, docs = filled
    lower = set(col.get(where_document={"$contains": "http"})["ids"])
    upper = set(col.get(where_document={"$contains": "HTTP"})["ids"])
    assert lower == {f"id{i}" for i in range(N) if docs[i] and "http" in docs[i]}
    assert upper == {f"id{i}" for i in range(N) if docs[i] and "HTTP" in docs[i]}
    assert lower != upper


@pytest.mark.parametrize("where", [{"namespace": "prod:api"}, {"namespace": {"$eq": "staging:api"}}, {"kind": "gauge"},
                                   {"$and": [{"namespace": "prod:billing"}, {"rank": {"$lt": 40}}]}, {"namespace": "nobody"}])
def test_where_and_where_document_must_both_hold(filled, where):
    from tests.test_where_facade import passes as md_passes

    col, vecs, docs = filled
    q = np.random.default_rng(4).standard_normal((2, DIM)).astype(np.float32)
    wd = {"$contains": "e"}
    out = col.query(query_embeddings=q, n_results=6, where=where, where_document=wd)
    for b in range(2):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 6, also=lambda i: md_passes(metadata_of(i), where))
        assert out["ids"][b] == ids and out["distances"][b] == dist


def test_a_where_list_per_query_combines_with_the_one_document_filter(filled):
    from tests.test_where_facade import passes as md_passes

    col, vecs, docs = filled
    q = np.random.default_rng(5).standard_normal((3, DIM)).astype(np.float32)
    wheres = [None, {"namespace": "prod:api"}, {"rank": {"$gte": 30}}]
    wd = {"$not_contains": "rate"}
    out = col.query(query_embeddings=q, n_results=4, where=wheres, where_document=wd)
    for b, w in enumerate(wheres):
        ids, dist = expected(vecs, docs, range(N), q[b], wd, 4, also=lambda i: w is None or md_passes(metadata_of(i), w))
        assert out["ids"][b] == ids and out["distances"][b] == dist


def test_get_filters_by_document_with_where_and_with_ids(filled):
    col, _, docs = filled
    wd = {"$or": [{"$contains": "queue"}, {"$contains": "latency"}]}
    want = [f"id{i}" for i in range(N) if passes(docs[i], wd)]
    assert col.get(where_document=wd)["ids"] == want
    assert col.get(where_document=wd, limit=3, offset=2)["ids"] == want[2:5]
    asked = ["id3", "id0", "nobody", "id9", "id8"]
    assert col.get(ids=asked, where_document=wd)["ids"] == [i for i in asked if i in want]
    both = col.get(where={"kind": "gauge"}, where_document=wd)["ids"]
    assert both == [i for i in want if int(i[2:]) % 2]


BAD = [
    ({"$contains": ""}, "non-empty str"),
    ({"$not_contains": ""}, "non-empty str"),
    ({"$contains": 5}, "non-empty str"),
    ({"$contains": None}, "non-empty str"),
    ({"$contains": ["a"]}, "non-empty str"),
    ({"$regex": "a.*"}, "unknown operator '$regex'"),
    ({"contains": "a"}, "unknown operator 'contains'"),
    ({"$and": []}, "$and takes a non-empty list"),
    ({"$or": {"$contains": "a"}}, "$or takes a non-empty list"),
    ({"$and": [{"$contains": "a"}, {"$contains": ""}]}, "non-empty str"),
    ({"$contains": "a", "$not_contains": "b"}, "exactly one key"),
    ({}, "exactly one key"),
    ("latency", "exactly one key"),
    ([{"$contains": "a"}], "exactly one key"),               # one filter per call: no list per query
]


@pytest.mark.parametrize("wd,why", BAD, ids=[str(i) for i in range(len(BAD))])
def test_anything_outside_the_grammar_is_a_value_error_that_names_the_supported_forms(filled, wd, why):
    col, _, _ = filled
    q = np.zeros((1, DIM), dtype=np.float32)
    for call in (lambda: col.query(query_embeddings=q, where_document=wd), lambda: col.get(where_document=wd)):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert "unsupported where_document filter" in msg and why in msg
        for form in ('{"$contains": "text"}', '{"$not_contains": "text"}', '{"$and": [filters]}', '{"$or": [filters]}'):
            assert form in msg


def test_an_engine_without_masked_search_raises_value_error():
    col = KnnClient(engine_factory=lambda dim: OracleEngine(dim)).get_or_create_collection("plain")
    col.upsert(ids=["a", "b"], embeddings=np.eye(2, DIM, dtype=np.float32), documents=["x", "y"])
    with pytest.raises(ValueError, match="no masked search"):
        col.query(query_embeddings=np.ones((1, DIM), dtype=np.float32), where_document={"$contains": "x"})


def test_the_host_path_goes_through_search_masked_once_per_call(filled):
    col, _, docs = filled
    engine = col._engine
    before = len(engine.masks)
    col.query(query_embeddings=np.ones((4, DIM), dtype=np.float32), n_results=3, where_document={"$contains": "queue"})
    assert len(engine.masks) == before + 1
    assert engine.masks[-1].tolist() == [docs[i] is not None and "queue" in docs[i] for i in range(N)]


def test_upsert_delete_and_compact_drop_the_caches():
    col = masked_client().get_or_create_collection("churn")
    vecs = fill(col, n=30)
    docs = [document_of(i) for i in range(30)]
    wd = {"$contains": "latency"}
    q = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)

    def check(order):
        out = col.query(query_embeddings=q[None, :], n_results=5, where_document=wd)
        ids, dist = expected(vecs, docs, order, q, wd, 5)
        assert out["ids"][0] == ids and out["distances"][0] == dist
        assert col._doc_mask_cache

    check(range(30))
    # an upsert that rewrites a document: id1 gains the needle, id0 loses it
    assert "latency" in docs[0] and "latency" not in docs[1]
    docs[0], docs[1] = "nothing to see", "latency at last"
    col.upsert(ids=["id0", "id1"], embeddings=vecs[[0, 1]], documents=[docs[0], docs[1]])
    assert not col._doc_mask_cache and not col._doc_bits_cache and not col._docs_on_device
    check(range(30))
    col.delete(ids=["id9", "id18"])                          # "latency" documents (i % 9 == 0)
    assert not col._doc_mask_cache
    live = [i for i in range(30) if i not in (9, 18)]
    check(live)
    assert "id9" not in col.get(where_document=wd)["ids"]
    col.compact()
    assert not col._doc_mask_cache
    check(live)                                              # slots renumbered, the same answers


def store_with_metrics():
    store = MetricsSemanticMetadataStore(masked_client(), collection_name="metrics")
    store.index_metadata("prod:api", {"metric_name": "http.latency", "description": "HTTP request latency in milliseconds", "unit": "ms"})
    store.index_metadata("prod:api", {"metric_name": "http.errors", "description": "HTTP 5xx responses", "category": "errors"})
    store.index_metadata("prod:db", {"metric_name": "db.query.time", "description": "Database query latency", "category": "database"})
    store.index_metadata("prod:db", {"metric_name": "db.pool.size", "description": "Connections in the pool"})
    return store


def test_the_store_and_the_search_client_pass_where_document_straight_through():
    store = store_with_metrics()
    hits = store.search_metadata("latency", n_results=10, where_document={"$contains": "HTTP"})
    assert sorted(h["metric_name"] for h in hits) == ["http.errors", "http.latency"]
    hits = store.search_metadata("latency", n_results=10, namespace="prod:db", where_document={"$contains": "latency"})
    assert [h["metric_name"] for h in hits] == ["db.query.time"]
    batch = store.search_metadata_batch(["latency", "", "pool"], n_results=10, where_document={"$not_contains": "HTTP"})
    assert [sorted(h["metric_name"] for h in r) for r in batch] == [["db.pool.size", "db.query.time"], [], ["db.pool.size", "db.query.time"]]
    client = MetricsSearchClient(store)
    found = client.search_relevant_metrics("request latency", limit=5, where_document={"$contains": "milliseconds"})
    assert [h["metric_name"] for h in found] == ["http.latency"]
    found = client.search_relevant_metrics("anything", limit=5, where={"category": "errors"}, where_document={"$contains": "5xx"})
    assert [h["metric_name"] for h in found] == ["http.errors"]
    many = client.search_relevant_metrics_batch(["latency", "errors"], limit=5, namespace=["prod:api", "prod:db"],
                                                where_document={"$contains": "latency"})
    assert [[h["metric_name"] for h in r] for r in many] == [["http.latency"], ["db.query.time"]]
    with pytest.raises(ValueError, match="unsupported where_document filter"):
        client.search_relevant_metrics("latency", where_document={"$contains": ""})
