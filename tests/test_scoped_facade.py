"""Namespace-scoped search above the engine, on a checker engine (tests/_scoped_oracle_engine.py): `where=` of the chromadb-shaped
façade, `namespace=` of the store and of MetricsSearchClient, the wire shims, reload from disk and a two-rank gloo
ShardedSearcher with scopes; plus what the C ABI's two scope entry points answer without a device.  No GPU."""

import asyncio
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from fastapi.testclient import TestClient

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore, native
from codd_query_engine_amd.sharded import ShardedSearcher, shard_bounds
from codd_query_engine_amd.wire import MetricsSearchRequest, cli_main, create_app, make_search_relevant_metrics_tool
from oracle import knn_oracle as o
from tests._oracle_engine import OracleEngine
from tests._scoped_oracle_engine import ScopedOracleEngine, scoped_reference

NAMESPACES = ["prod:api", "staging:api", "prod:billing"]


def scoped_client(**kw):
    return KnnClient(engine_factory=lambda dim: ScopedOracleEngine(dim), **kw)


def fill(col, n=60, dim=48, seed=3):
    """n rows, namespaces dealt round-robin, every fifth row without one; returns (vectors, namespace or None per row)."""
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    ns = [None if i % 5 == 4 else NAMESPACES[i % 3] for i in range(n)]
    md = [None if i % 10 == 9 else ({"k": i} if ns[i] is None else {"k": i, "namespace": ns[i]}) for i in range(n)]
    col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=md, documents=[f"doc {i}" for i in range(n)])
    return vecs, ns


def expected_ids(vecs, ns, q, namespace, k):
    """Brute force through the oracle over the namespace's sub-matrix."""
    members = np.array([i for i, x in enumerate(ns) if x == namespace], dtype=np.int64)
    if members.size == 0:
        return [], []
    d, i = o.search(o.normalize_rows(vecs[members]), "f32", o.normalize_rows(q[None, :]), min(k, len(ns)))
    hit = i[0] >= 0
    return [f"id{members[j]}" for j in i[0][hit]], d[0][hit].tolist()


def test_where_returns_the_exact_top_k_of_one_namespace():
    col = scoped_client().get_or_create_collection("c")
    vecs, ns = fill(col)
    q = np.random.default_rng(9).standard_normal(48).astype(np.float32)
    for form in ({"namespace": "prod:api"}, {"namespace": {"$eq": "prod:api"}}):
        out = col.query(query_embeddings=q, n_results=7, where=form)
        ids, dists = expected_ids(vecs, ns, q, "prod:api", 7)
        assert out["ids"] == [ids] and out["distances"] == [dists]
        assert all(m["namespace"] == "prod:api" for m in out["metadatas"][0])
        assert out["documents"][0] == [f"doc {int(i[2:])}" for i in ids]
    # a namespace with fewer rows than n_results returns what it has; n_results is still capped by count()
    out = col.query(query_embeddings=q, n_results=1000, where={"namespace": "prod:billing"})
    assert sorted(out["ids"][0]) == sorted(f"id{i}" for i, x in enumerate(ns) if x == "prod:billing")


def test_where_forms_that_are_not_supported_raise_value_error():
    col = scoped_client().get_or_create_collection("c")
    fill(col)
    q = np.zeros(48, dtype=np.float32) + 1
    for bad in ({"category": "x"}, {"namespace": {"$in": ["a", "b"]}}, {"namespace": "a", "category": "b"}, {"namespace": 3},
                {"$and": [{"namespace": "a"}]}, "prod:api", {}, [{"namespace": "a"}, None]):
        with pytest.raises(ValueError, match="namespace"):
            col.query(query_embeddings=q, n_results=3, where=bad)


def test_unknown_namespace_gives_an_empty_inner_list_and_lists_mix_per_query():
    col = scoped_client().get_or_create_collection("c")
    vecs, ns = fill(col)
    rng = np.random.default_rng(11)
    q = rng.standard_normal((4, 48)).astype(np.float32)
    out = col.query(query_embeddings=q[:1], n_results=5, where={"namespace": "nobody"})
    assert out["ids"] == [[]] and out["distances"] == [[]] and out["metadatas"] == [[]] and out["documents"] == [[]]
    where = [{"namespace": "staging:api"}, None, {"namespace": "nobody"}, {"namespace": {"$eq": "prod:billing"}}]
    out = col.query(query_embeddings=q, n_results=5, where=where)
    plain = col.query(query_embeddings=q, n_results=5)
    assert out["ids"][0] == expected_ids(vecs, ns, q[0], "staging:api", 5)[0]
    assert out["ids"][1] == plain["ids"][1] and out["distances"][1] == plain["distances"][1]
    assert out["ids"][2] == []
    assert out["ids"][3] == expected_ids(vecs, ns, q[3], "prod:billing", 5)[0]
    # a list of None only is today's call
    eng = col._engine
    eng.calls.clear()
    assert col.query(query_embeddings=q, n_results=5, where=[None] * 4) == plain
    assert eng.calls == ["search"]


def test_where_none_is_the_same_call_as_before():
    col = scoped_client().get_or_create_collection("c")
    fill(col)
    q = np.random.default_rng(5).standard_normal((3, 48)).astype(np.float32)
    eng = col._engine
    eng.calls.clear()
    a = col.query(query_embeddings=q, n_results=4)
    b = col.query(query_embeddings=q, n_results=4, where=None)
    assert a == b and eng.calls == ["search", "search"]


def test_scopes_follow_the_metadata_through_rewrites():
    col = scoped_client().get_or_create_collection("c")
    vecs, ns = fill(col, n=20)
    eng = col._engine
    assert col._scope_of_namespace == {"prod:api": 1, "staging:api": 2, "prod:billing": 3}     # first seen first, from 1
    labels = [0 if x is None else col._scope_of_namespace[x] for x in ns]
    assert eng._labels().tolist() == labels
    # a vector rewritten without metadata keeps its namespace; new metadata moves it; metadata without the key clears it
    col.upsert(ids=["id0"], embeddings=vecs[3:4])
    assert eng._labels()[0] == labels[0]
    col.upsert(ids=["id0"], embeddings=vecs[3:4], metadatas=[{"namespace": "team:new"}])
    assert eng._labels()[0] == 4 and col._scope_of_namespace["team:new"] == 4
    col.upsert(ids=["id0"], embeddings=vecs[3:4], metadatas=[{"k": 1}])
    assert eng._labels()[0] == 0
    out = col.query(query_embeddings=vecs[3], n_results=20, where={"namespace": "team:new"})
    assert out["ids"] == [[]]
    # add() labels the rows it writes and leaves present ids alone
    col.add(ids=["id1", "fresh"], embeddings=vecs[:2], metadatas=[{"namespace": "zzz"}, {"namespace": "team:new"}])
    assert eng._labels()[1] == labels[1] and eng._labels()[20] == 4
    assert col.query(query_embeddings=vecs[0], n_results=5, where={"namespace": "team:new"})["ids"] == [["fresh"]]


def test_engine_without_scoped_search_is_never_asked_on_the_write_path_and_refuses_where():
    class Recording(OracleEngine):
        def __getattr__(self, name):  # any attribute the protocol of today does not have
            raise AttributeError(name)

    col = KnnClient(engine_factory=lambda dim: Recording(dim)).get_or_create_collection("c")
    vecs, _ = fill(col)
    plain = col.query(query_embeddings=vecs[0], n_results=3)
    assert plain["ids"][0][0] == "id0"
    with pytest.raises(NotImplementedError, match="scoped search"):
        col.query(query_embeddings=vecs[0], n_results=3, where={"namespace": "prod:api"})


def test_reload_rebuilds_scopes_from_the_stored_metadata(tmp_path):
    writer = scoped_client(path=str(tmp_path))
    col = writer.get_or_create_collection("c")
    vecs, ns = fill(col)
    q = np.random.default_rng(2).standard_normal(48).astype(np.float32)
    before = col.query(query_embeddings=q, n_results=6, where={"namespace": "staging:api"})
    assert writer.persist() == 1
    manifest = open(os.path.join(tmp_path, "c", "gen-00000001", "manifest.json")).read()
    assert '"format_version": 1' in manifest and "scope" not in manifest           # the on-disk format knows nothing of scopes
    reader = scoped_client(path=str(tmp_path))
    again = reader.get_collection("c")
    assert again._scope_of_namespace == col._scope_of_namespace
    assert again._engine._labels().tolist() == col._engine._labels().tolist()
    assert again.query(query_embeddings=q, n_results=6, where={"namespace": "staging:api"}) == before
    assert before["ids"][0] == expected_ids(vecs, ns, q, "staging:api", 6)[0]


def metrics_store(factory=None):
    store = MetricsSemanticMetadataStore(KnnClient(engine_factory=factory or (lambda dim: ScopedOracleEngine(dim))))
    for ns in NAMESPACES:
        store.index_metadata(ns, {"metric_name": "http_request_duration_seconds", "description": f"HTTP request latency in seconds ({ns})",
                                  "category": "application", "golden_signal_type": "latency"})
        store.index_metadata(ns, {"metric_name": "node_memory_MemFree_bytes", "description": "Free memory in bytes", "category": "infrastructure"})
    store.index_metadata("prod:billing", {"metric_name": "invoice_latency_seconds", "description": "Invoice rendering latency", "category": "application"})
    return store


def test_store_and_search_client_keep_to_the_namespace():
    store = metrics_store()
    hits = store.search_metadata("high latency", n_results=10, namespace="staging:api")
    assert hits and {h["namespace"] for h in hits} == {"staging:api"} and len(hits) == 2
    assert hits[0]["metric_name"] == "http_request_duration_seconds"
    assert store.search_metadata("high latency", namespace="nobody") == []
    assert store.search_metadata("   ", namespace="prod:api") == []
    everything = store.search_metadata("high latency", n_results=10)
    assert len(everything) == 7 and store.search_metadata("high latency", n_results=10, namespace=None) == everything
    batch = store.search_metadata_batch(["high latency", "", "free memory", "latency"], n_results=10,
                                        namespace=["prod:billing", "prod:api", None, "nobody"])
    assert {h["namespace"] for h in batch[0]} == {"prod:billing"} and len(batch[0]) == 3
    assert batch[1] == [] and batch[3] == [] and len(batch[2]) == 7
    assert store.search_metadata_batch(["high latency"], n_results=10, namespace="prod:api") == [store.search_metadata("high latency", 10, "prod:api")]
    assert store.search_metadata_batch(["high latency", "x"], n_results=10) == [everything, store.search_metadata("x", 10)]
    client = MetricsSearchClient(store)
    got = client.search_relevant_metrics("high latency", limit=5, namespace="prod:billing")
    assert [g["metric_name"] for g in got] == [h["metric_name"] for h in store.search_metadata("high latency", 5, "prod:billing")]
    assert client.search_relevant_metrics("high latency", limit=5) == client.search_relevant_metrics("high latency", limit=5, namespace=None)
    both = client.search_relevant_metrics_batch(["high latency", "high latency"], limit=5, namespace=["prod:billing", None])
    assert both[0] == got and both[1] == client.search_relevant_metrics("high latency", limit=5)


def test_store_on_an_engine_without_scoped_search():
    store = metrics_store(lambda dim: OracleEngine(dim))
    assert len(store.search_metadata("high latency", n_results=10)) == 7
    with pytest.raises(NotImplementedError):
        store.search_metadata("high latency", namespace="prod:api")


def test_wire_shims_carry_the_namespace(capsys):
    client = MetricsSearchClient(metrics_store())
    assert MetricsSearchRequest(query="q").namespace is None
    api = TestClient(create_app(lambda: client))
    plain = api.post("/api/metrics/search", json={"query": "high latency", "limit": 10}).json()
    assert plain["count"] == 7
    scoped = api.post("/api/metrics/search", json={"query": "high latency", "limit": 10, "namespace": "prod:billing"}).json()
    assert scoped["count"] == 3 and [r["metric_name"] for r in scoped["results"]] == \
        [r["metric_name"] for r in client.search_relevant_metrics("high latency", limit=10, namespace="prod:billing")]
    sent = []

    def post(endpoint, body):
        sent.append(body)
        return api.post(endpoint, json=body).json()

    tool = make_search_relevant_metrics_tool(post)
    assert asyncio.run(tool("high latency", limit=10)) == plain["results"]
    assert asyncio.run(tool("high latency", limit=10, namespace="prod:billing")) == scoped["results"]
    assert sent == [{"query": "high latency", "limit": 10}, {"query": "high latency", "limit": 10, "namespace": "prod:billing"}]
    assert cli_main(["get-semantic-metrics", "high latency", "--limit", "10", "--namespace", "prod:billing"], search_client=client) == 0
    table = capsys.readouterr().out
    assert "Top 3" in table and "invoice_latency_seconds" in table
    assert cli_main(["get-semantic-metrics", "high latency", "--limit", "10"], search_client=client) == 0
    assert "Top 7" in capsys.readouterr().out


# ---- two ranks over gloo, scopes on every shard ---------------------------------------------------------------------

class TensorScopedEngine:
    def __init__(self, inner):
        self.inner = inner

    def search_keys(self, queries, k, row_base):
        return torch.from_numpy(self.inner.search_keys(np.asarray(queries), k, row_base).view(np.int64).copy())

    def search_keys_scoped(self, queries, scopes, k, row_base):
        return torch.from_numpy(self.inner.search_keys_scoped(np.asarray(queries), np.asarray(scopes), k, row_base).view(np.int64).copy())


def oracle_merge(keys_t, k):
    merged, d, r = OracleEngine.merge_keys(keys_t.numpy().view(np.uint64), k)
    return torch.from_numpy(merged.view(np.int64).copy()), torch.from_numpy(d), torch.from_numpy(r)


def sharded_data(n=601, d=64, B=6):
    rng = np.random.default_rng(41)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    scope_of = (rng.integers(0, 4, n)).astype(np.uint32)       # 0 = unlabelled, 1..3
    raw[n // 2 + 7] = raw[4]                                   # the same vector on both shards ...
    scope_of[4] = scope_of[n // 2 + 7] = 2                     # ... in one scope: the lower GLOBAL row wins
    q = rng.standard_normal((B, d)).astype(np.float32)
    q[0] = raw[4]
    scopes = np.array([2, 1, 0, 3, 9, 2], dtype=np.uint32)     # 9: a scope nobody carries
    return raw, scope_of, q, scopes


def gloo_worker(rank, world, port, k, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        raw, scope_of, q, scopes = sharded_data()
        lo, hi = shard_bounds(raw.shape[0], world, rank)
        eng = ScopedOracleEngine(raw.shape[1])
        eng.upsert(np.arange(hi - lo, dtype=np.int64), raw[lo:hi])
        eng.set_scopes(np.arange(hi - lo, dtype=np.int64), scope_of[lo:hi])
        searcher = ShardedSearcher(TensorScopedEngine(eng), row_base=lo, merge=oracle_merge)
        dd, rr = searcher.search(q, k, scopes=scopes)
        dd2, rr2 = searcher.search_async(q, k, scopes=scopes).result()
        assert torch.equal(dd, dd2) and torch.equal(rr, rr2)
        du, ru = searcher.search(q, k)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), dist=dd.numpy(), rows=rr.numpy(), dist_u=du.numpy(), rows_u=ru.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_search_with_scopes(tmp_path):
    k = 8
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(gloo_worker, args=(2, port, k, str(tmp_path)), nprocs=2, join=True)
    raw, scope_of, q, scopes = sharded_data()
    rows_ref, qn = o.normalize_rows(raw), o.normalize_rows(q)
    d_ref, r_ref = scoped_reference(rows_ref, "f32", scope_of, qn, scopes, k)
    d_all, r_all = o.search(rows_ref, "f32", qn, k)
    for rank in range(2):
        got = np.load(tmp_path / f"rank{rank}.npz")
        assert np.array_equal(got["rows"], r_ref) and np.array_equal(got["dist"], d_ref), rank
        assert np.array_equal(got["rows_u"], r_all) and np.array_equal(got["dist_u"], d_all), rank
    assert r_ref[0, 0] == 4 and r_ref[0, 1] == raw.shape[0] // 2 + 7
    assert (r_ref[4] == -1).all() and np.array_equal(r_ref[2], r_all[2])


# ---- the C ABI without a device -------------------------------------------------------------------------------------

def test_scope_entry_points_validate_before_any_hip_call():
    lib = native.load()
    assert lib.codd_knn_search_scoped(None, None, None, 1, 1, 0, None, None, None, None) == -22
    assert "null" in native.last_error()
    assert lib.codd_knn_set_scopes_host(None, None, None, 0) == -22
    assert lib.codd_knn_set_scopes_host(None, None, None, 5) == -22
    assert native.MAX_SCOPE == 1048575
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_knn.h")).read()
    assert "#define CODD_KNN_MAX_SCOPE 1048575u" in header
    names = [name for name, _, _ in native.ABI]
    assert "codd_knn_search_scoped" in names and "codd_knn_set_scopes_host" in names
    assert isinstance(ctypes.c_uint32(native.MAX_SCOPE).value, int)
