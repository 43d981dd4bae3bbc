"""A general `where` above the engine, on a checker engine with search_masked (tests/_masked_oracle_engine.py):
ChromaDB's metadata grammar through Collection.query / Collection.get, the store's and MetricsSearchClient's `where=`, the
routing of a per-query list, the malformed forms, and the cache of compiled masks across upsert / delete / compact.  The
expected ids of every query come from a plain Python evaluation of the filter over this file's own metadata and the oracle on the
rows that pass.  No GPU."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore
from oracle import knn_oracle as o
from tests._masked_oracle_engine import MaskedOracleEngine

DIM = 48
N = 90
NAMESPACES = ["prod:api", "staging:api", "prod:billing"]
TYPES = ["counter", "gauge", "histogram"]


def masked_client(**kw):
    return KnnClient(engine_factory=lambda dim: MaskedOracleEngine(dim), **kw)


def metadata_of(i: int):
    """Record i's metadata: every tenth record has none, every seventh lacks "type", "weight" is a float on even records only."""
    if i % 10 == 9:
        return None
    md = {"namespace": NAMESPACES[i % 3], "rank": i, "hot": i % 4 == 0, "unit": "seconds" if i % 2 else 7}
    if i % 7:
        md["type"] = TYPES[i % 3 if i % 5 else (i + 1) % 3]
    if i % 2 == 0:
        md["weight"] = i / 8.0
    return md


def fill(col, n=N, seed=5):
    vecs = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=[metadata_of(i) for i in range(n)])
    return vecs


def cls(v):
    return "b" if isinstance(v, bool) else "n" if isinstance(v, (int, float)) else "s"


def passes(md, where) -> bool:
    """The filter's meaning, record by record (the rules of the issue: a missing key fails $eq / $in / comparisons and passes
    $ne / $nin; values of different classes never compare)."""
    (key, cond), = where.items()
    if key == "$and":
        return all(passes(md, w) for w in cond)
    if key == "$or":
        return any(passes(md, w) for w in cond)
    (op, val), = (cond if isinstance(cond, dict) else {"$eq": cond}).items()
    has = md is not None and key in md
    same = lambda a, b: cls(a) == cls(b) and a == b  # noqa: E731
    if op == "$eq":
        return has and same(md[key], val)
    if op == "$ne":
        return not (has and same(md[key], val))
    if op == "$in":
        return has and any(same(md[key], v) for v in val)
    if op == "$nin":
        return not (has and any(same(md[key], v) for v in val))
    if not has or cls(md[key]) != cls(val):
        return False
    return {"$gt": md[key] > val, "$gte": md[key] >= val, "$lt": md[key] < val, "$lte": md[key] <= val}[op]


def expected(vecs, mds, order, q, where, k):
    """(ids, distances) of one query: the oracle over the records of `order` (tie order) whose metadata passes."""
    keep = [i for i in order if where is None or passes(mds[i], where)]
    if not keep:
        return [], []
    k = min(k, len(order))
    d, i = o.search(o.normalize_rows(vecs[keep]), "f32", o.normalize_rows(q[None, :]), k)
    hit = i[0] >= 0
    return [f"id{keep[j]}" for j in i[0][hit]], d[0][hit].tolist()


FILTERS = [
    {"type": "gauge"},
    {"type": {"$eq": "histogram"}},
    {"type": {"$ne": "counter"}},                                  # records without "type" (and without metadata) pass
    {"rank": {"$gt": 40}},
    {"rank": {"$gte": 40}},
    {"rank": {"$lt": 13}},
    {"rank": {"$lte": 13}},
    {"weight": {"$gt": 2.5}},                                      # a float key only even records carry
    {"weight": {"$lte": 3}},                                       # int against stored floats
    {"rank": {"$eq": 12.0}},                                       # float against a stored int
    {"hot": True},
    {"hot": {"$ne": True}},
    {"hot": 1},                                                    # a number is not a bool: nobody
    {"unit": 7},
    {"unit": {"$gt": 3}},                                          # the str values of "unit" never compare with a number
    {"unit": {"$gt": "a"}},
    {"type": {"$in": ["counter", "histogram"]}},
    {"type": {"$nin": ["counter", "histogram"]}},                  # missing keys pass
    {"rank": {"$in": [3, 4, 5, 400]}},
    {"namespace": {"$in": ["prod:api", "prod:billing"]}},
    {"namespace": {"$ne": "staging:api"}},                         # "everything except staging"
    {"$and": [{"namespace": "prod:api"}, {"type": {"$in": ["counter", "histogram"]}}]},
    {"$or": [{"type": "gauge"}, {"rank": {"$lt": 5}}]},
    {"$and": [{"$or": [{"hot": True}, {"weight": {"$gte": 8}}]}, {"namespace": {"$ne": "prod:billing"}}, {"rank": {"$gt": 10}}]},
    {"$or": [{"$and": [{"type": "counter"}, {"hot": False}]}, {"$and": [{"unit": "seconds"}, {"rank": {"$lte": 20}}]}]},
    {"type": "no-such-type"},                                      # nobody matches
    {"no_such_key": {"$gt": 0}},
    {"no_such_key": {"$ne": 0}},                                   # everybody matches
]


@pytest.fixture(scope="module")
def filled():
    col = masked_client().get_or_create_collection("c")
    vecs = fill(col)
    return col, vecs, [metadata_of(i) for i in range(N)]


@pytest.mark.parametrize("where", FILTERS, ids=[str(i) for i in range(len(FILTERS))])
def test_every_operator_against_the_plain_evaluation(filled, where):
    col, vecs, mds = filled
    rng = np.random.default_rng(9)
    q = rng.standard_normal((3, DIM)).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=6, where=where)
    for b in range(3):
        ids, dists = expected(vecs, mds, list(range(N)), q[b], where, 6)
        assert out["ids"][b] == ids and out["distances"][b] == dists, (where, b)
        assert out["metadatas"][b] == [mds[int(i[2:])] for i in ids]
    got = col.get(where=where)["ids"]
    assert got == [f"id{i}" for i in range(N) if passes(mds[i], where)], where


def test_nobody_matching_gives_an_empty_inner_list_and_no_engine_call(filled):
    col, _, _ = filled
    calls = len(col._engine.calls)
    out = col.query(query_embeddings=np.ones((2, DIM), dtype=np.float32), n_results=4, where={"type": "no-such-type"})
    assert out["ids"] == [[], []] and out["distances"] == [[], []] and out["metadatas"] == [[], []] and out["documents"] == [[], []]
    assert len(col._engine.calls) == calls


def test_get_combines_where_with_ids_limit_and_offset(filled):
    col, _, mds = filled
    where = {"type": "gauge"}
    gauges = [f"id{i}" for i in range(N) if passes(mds[i], where)]
    assert col.get(where=where, limit=4, offset=2)["ids"] == gauges[2:6]
    assert col.get(ids=["id3", gauges[0], "never", gauges[5]], where=where)["ids"] == [i for i in ("id3", gauges[0], gauges[5]) if i in gauges]
    assert col.get(where={"namespace": "prod:api"})["ids"] == [f"id{i}" for i in range(N) if mds[i] and mds[i]["namespace"] == "prod:api"]


def test_a_mixed_list_goes_to_plain_scoped_and_masked_calls_grouped_by_filter():
    col = masked_client().get_or_create_collection("c")
    vecs = fill(col)
    mds = [metadata_of(i) for i in range(N)]
    rng = np.random.default_rng(13)
    q = rng.standard_normal((7, DIM)).astype(np.float32)
    general, other = {"type": {"$in": ["gauge", "histogram"]}}, {"rank": {"$lt": 30}}
    where = [None, {"namespace": "prod:api"}, general, {"namespace": {"$eq": "nobody"}}, other, dict(general), {"type": "no-such-type"}]
    col._engine.calls.clear()
    out = col.query(query_embeddings=q, n_results=5, where=where)
    for b, w in enumerate(where):
        ids, dists = expected(vecs, mds, list(range(N)), q[b], w, 5)
        assert out["ids"][b] == ids and out["distances"][b] == dists, (b, w)
    assert sorted(col._engine.calls) == ["search", "search_masked", "search_masked", "search_scoped"], "one call per distinct filter"
    assert out["ids"][3] == [] and out["ids"][6] == []
    # namespace-only filters keep to the scoped call alone
    col._engine.calls.clear()
    col.query(query_embeddings=q[:2], n_results=5, where=[{"namespace": "prod:api"}, None])
    assert col._engine.calls == ["search_scoped"]


def test_a_filter_over_deleted_records_and_the_cache_follows_upsert_delete_and_compact():
    col = masked_client().get_or_create_collection("c")
    vecs = fill(col)
    mds = [metadata_of(i) for i in range(N)]
    q = np.random.default_rng(17).standard_normal(DIM).astype(np.float32)
    where = {"$and": [{"type": {"$ne": "counter"}}, {"rank": {"$lt": 60}}]}
    order = list(range(N))

    def agree(what):
        out = col.query(query_embeddings=q, n_results=8, where=where)
        ids, dists = expected(vecs, mds, order, q, where, 8)
        assert out["ids"] == [ids] and out["distances"] == [dists], what
        assert col.get(where=where)["ids"] == [f"id{i}" for i in order if passes(mds[i], where)], what
        return ids

    first = agree("fresh")
    assert agree("cached") == first and len(col._mask_cache) == 1
    # delete the two best matches: the cached mask must not bring them back
    gone = [int(first[0][2:]), int(first[1][2:])]
    col.delete(ids=[f"id{g}" for g in gone])
    order = [i for i in order if i not in gone]
    second = agree("after delete")
    assert second != first and not set(second) & {f"id{g}" for g in gone}
    assert not col._engine.masks[-1][gone].any(), "deleted slots are False in the mask"
    # rewrite a record's metadata so that it stops matching, and one so that it starts to
    leaves, joins = int(second[0][2:]), next(i for i in order if not passes(mds[i], where) and mds[i] is not None)
    mds[leaves] = dict(mds[leaves], type="counter")
    mds[joins] = {"rank": 1, "type": "gauge", "namespace": "prod:api"}
    vecs[joins] = q                                                # ... as the best match
    col.upsert(ids=[f"id{leaves}", f"id{joins}"], embeddings=vecs[[leaves, joins]], metadatas=[mds[leaves], mds[joins]])
    third = agree("after upsert")
    assert third[0] == f"id{joins}" and f"id{leaves}" not in third
    # compaction renumbers the slots: a mask cached before it would name the wrong rows
    assert col.compact() == len(order) and col._engine.compactions == 1
    assert agree("after compact") == third
    assert col._engine.masks[-1].shape == (len(order),)


def test_malformed_filters_raise_value_error(filled):
    col, _, _ = filled
    q = np.ones(DIM, dtype=np.float32)
    bad = [{}, {"type": "gauge", "rank": 3}, {"type": {"$eq": "a", "$ne": "b"}}, {"type": {"$like": "a"}}, {"$not": [{"type": "a"}]},
           {"$and": []}, {"$or": []}, {"$and": {"type": "a"}}, {"type": {"$in": []}}, {"type": {"$nin": "gauge"}}, {"type": None},
           {"type": ["gauge"]}, {"type": {"$eq": {"a": 1}}}, {"type": {"$in": ["a", None]}}, {"$and": [{"type": "a"}, {"rank": {"$between": 3}}]},
           "gauge", {3: "a"}]
    for where in bad:
        with pytest.raises(ValueError, match="where"):
            col.query(query_embeddings=q, n_results=3, where=where)
        with pytest.raises(ValueError, match="where"):
            col.get(where=where)
    with pytest.raises(ValueError, match="where"):
        col.query(query_embeddings=q, n_results=3, where=[{"type": "gauge"}, None])      # two filters for one query
    with pytest.raises(ValueError, match="namespace"):
        col.delete(where={"type": "gauge"})                                              # delete keeps its namespace-only grammar


def metrics_store():
    store = MetricsSemanticMetadataStore(masked_client())
    for ns in NAMESPACES:
        store.index_metadata(ns, {"metric_name": "http_request_duration_seconds", "description": f"HTTP request latency in seconds ({ns})",
                                  "type": "histogram", "category": "application", "golden_signal_type": "latency"})
        store.index_metadata(ns, {"metric_name": "http_requests_total", "description": "HTTP requests served", "type": "counter",
                                  "category": "application", "golden_signal_type": "traffic"})
        store.index_metadata(ns, {"metric_name": "node_memory_MemFree_bytes", "description": "Free memory in bytes", "type": "gauge",
                                  "category": "infrastructure"})
    return store


def test_where_through_the_store_and_the_search_client_alone_and_with_namespace():
    store = metrics_store()
    client = MetricsSearchClient(store)
    plain = store.search_metadata("request latency", 9)
    assert len(plain) == 9
    latency = store.search_metadata("request latency", 9, where={"golden_signal_type": "latency"})
    assert [h["metric_name"] for h in latency] == ["http_request_duration_seconds"] * 3
    assert [(h["metric_name"], h["namespace"]) for h in latency] == [(h["metric_name"], h["namespace"]) for h in plain if h.get("golden_signal_type") == "latency"]
    both = store.search_metadata("request latency", 9, namespace="prod:api", where={"type": {"$in": ["counter", "histogram"]}})
    assert sorted(h["metric_name"] for h in both) == ["http_request_duration_seconds", "http_requests_total"]
    assert {h["namespace"] for h in both} == {"prod:api"}
    assert [(h["metric_name"], h["similarity_score"]) for h in both] == [
        (h["metric_name"], h["similarity_score"]) for h in plain if h["namespace"] == "prod:api" and h["type"] in ("counter", "histogram")]
    assert store.search_metadata("request latency", 9, namespace="prod:api", where={"type": "no-such-type"}) == []
    got = client.search_relevant_metrics("request latency", limit=9, namespace="staging:api", where={"category": {"$ne": "infrastructure"}})
    assert sorted(g["metric_name"] for g in got) == ["http_request_duration_seconds", "http_requests_total"]
    assert client.search_relevant_metrics("request latency", limit=9, where={"golden_signal_type": "latency"}) == [
        {k: v for k, v in g.items()} for g in client.search_relevant_metrics("request latency", limit=9) if g["golden_signal_type"] == "latency"]
    batch = client.search_relevant_metrics_batch(["request latency", "", "free memory"], limit=9, namespace=["prod:api", None, None],
                                                 where={"type": {"$ne": "counter"}})
    assert batch[1] == [] and {g["metric_name"] for g in batch[0]} == {"http_request_duration_seconds", "node_memory_MemFree_bytes"}
    assert len(batch[0]) == 2 and len(batch[2]) == 6
    assert batch[2] == client.search_relevant_metrics("free memory", limit=9, where={"type": {"$ne": "counter"}})
    # the reference's own call shapes reach the engine as before: a plain search, nothing masked
    store.collection._engine.calls.clear()
    client.search_relevant_metrics("request latency", limit=3)
    client.search_relevant_metrics("request latency", limit=3, namespace="prod:api")
    assert store.collection._engine.calls == ["search", "search_scoped"]
