"""Namespace-scoped search on the GPU (codd_knn_set_scopes_host / codd_knn_search_scoped).  The reference for a
query of scope s is the oracle's search over the sub-matrix rows[scope_of == s] (row order kept, so "ties -> lower row" carries
over) with the indices mapped back through np.flatnonzero; scope 0 is the whole matrix.  Every comparison is bit for bit on row
ids and fp32 distances: no tolerance, no case left out."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests._scoped_oracle_engine import scoped_reference

pytestmark = pytest.mark.gpu

SIZES = [5, 37, 500, 2000, 4000, 6000, 5000]      # rows of scopes 1 .. 7 (scope 1 holds fewer than k = 10 rows); the rest stay at scope 0
N = 20_000
UNKNOWN = [99, native.MAX_SCOPE, 4_000_000_000]   # above anything ever set, the largest legal label, past the legal range


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def labels_mixed(n, sizes, seed):
    """scope label per row: sizes[s-1] rows of scope s at random positions, 0 elsewhere."""
    lab = np.zeros(n, dtype=np.uint32)
    lab[: sum(sizes)] = np.repeat(np.arange(1, len(sizes) + 1, dtype=np.uint32), sizes)
    return np.random.default_rng(seed).permutation(lab)


def build(Index, raw, dtype, labels):
    ix = Index(raw.shape[1], dtype=dtype)
    n = raw.shape[0]
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ix.set_scopes(np.arange(n, dtype=np.int64), labels)
    return ix


def stored(raw, dtype):
    return o.to_storage(o.normalize_rows(raw), dtype)


def check(ix, rows_ref, dtype, labels, q, scopes, k):
    d_ref, r_ref = scoped_reference(rows_ref, dtype, labels, o.normalize_rows(q), scopes, k)
    dist, rows = ix.search_scoped(q, scopes, k)
    assert np.array_equal(rows, r_ref), (dtype, q.shape, k, np.flatnonzero((rows != r_ref).any(axis=1))[:8])
    assert np.array_equal(dist, d_ref), (dtype, q.shape, k)
    return dist, rows


@pytest.mark.parametrize("dtype,dim", [("f32", 384), ("f32", 768), ("bf16", 384), ("bf16", 768), ("f16", 384), ("f16", 768),
                                       ("f32", 1536), ("f32", 100), ("bf16", 2048), ("f16", 3072), ("f32", 1024), ("f16", 2048)])
def test_scoped_search_equals_the_oracle_on_the_sub_matrix(Index, dtype, dim):
    rng = np.random.default_rng(dim + len(dtype))
    raw = rng.standard_normal((N, dim)).astype(np.float32)
    labels = labels_mixed(N, SIZES, seed=dim)
    ix = build(Index, raw, dtype, labels)
    rows_ref = stored(raw, dtype)
    assert ix.stat("scopes") == 7 and ix.stat("scope_builds") == 0
    cycle = np.array(list(range(1, 8)) + [0] + UNKNOWN, dtype=np.uint32)
    searches = 0
    for B in (1, 5, 64, 256):
        q = rng.standard_normal((B, dim)).astype(np.float32)
        q[0] = raw[int(np.flatnonzero(labels == 4)[0])]                 # a query equal to a stored row of its scope
        scopes = np.resize(np.roll(cycle, -3), B) if B > 1 else np.array([4], dtype=np.uint32)
        for k in (1, 10, 100):
            dist, rows = check(ix, rows_ref, dtype, labels, q, scopes, k)
            searches += 1
            for b in np.flatnonzero(scopes == 0)[:2]:                   # scope 0 = every row: the bits of ix.search
                d_all, r_all = ix.search(q[b : b + 1], k)
                assert np.array_equal(rows[b], r_all[0]) and np.array_equal(dist[b], d_all[0])
            for b in np.flatnonzero(np.isin(scopes, UNKNOWN)):
                assert (rows[b] == -1).all() and np.isinf(dist[b]).all()
            for b in np.flatnonzero(scopes == 1):                       # 5 rows: padding behind them
                assert (rows[b, : min(k, 5)] >= 0).all() and (rows[b, 5:] == -1).all()
    # a single query in each scope, the unknown ones and scope 0 included (one work item, the list cut into parts)
    q1 = rng.standard_normal((1, dim)).astype(np.float32)
    for s in cycle:
        check(ix, rows_ref, dtype, labels, q1, np.array([s], dtype=np.uint32), 10)
        searches += 1
    assert ix.stat("scoped_searches") == searches and ix.stat("scope_builds") == 1     # the lists are built once
    ix.close()


def test_ties_inside_a_scope_and_across_scopes(Index):
    rng = np.random.default_rng(5)
    n, dim = 6000, 384
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    labels = (np.arange(n) % 3 + 1).astype(np.uint32)
    v = rng.standard_normal(dim).astype(np.float32)
    dup = [10, 13, 1000, 4000, 11, 2000]     # scope 2: rows 10, 13, 1000, 4000; scope 3: rows 11, 2000
    raw[dup] = v
    assert labels[dup].tolist() == [2, 2, 2, 2, 3, 3]
    ix = build(Index, raw, "f32", labels)
    rows_ref = stored(raw, "f32")
    q = np.stack([v, v, v, v])
    scopes = np.array([2, 3, 1, 0], dtype=np.uint32)
    dist, rows = check(ix, rows_ref, "f32", labels, q, scopes, 10)
    assert rows[0, :4].tolist() == [10, 13, 1000, 4000] and not set(rows[0].tolist()) & {11, 2000}
    assert rows[1, :2].tolist() == [11, 2000] and not set(rows[1].tolist()) & {10, 13, 1000, 4000}
    assert not set(rows[2].tolist()) & set(dup)
    assert rows[3, :6].tolist() == sorted(dup)
    assert len({dist[0, j] for j in range(4)} | {dist[1, 0], dist[1, 1]}) == 1
    ix.close()


def test_contiguous_and_round_robin_layouts_give_the_same_results(Index):
    rng = np.random.default_rng(6)
    n, dim, ns = 12_000, 768, 12
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rr = (np.arange(n) % ns + 1).astype(np.uint32)                       # round-robin: a scope's rows 12 slots apart
    order = np.argsort(rr, kind="stable")                                # the same (vector, scope) pairs, each scope in one run
    ix_rr, ix_ct = build(Index, raw, "f32", rr), build(Index, raw[order], "f32", rr[order])
    q = rng.standard_normal((40, dim)).astype(np.float32)
    scopes = (np.arange(40) % ns + 1).astype(np.uint32)
    d_rr, r_rr = check(ix_rr, stored(raw, "f32"), "f32", rr, q, scopes, 10)
    d_ct, r_ct = check(ix_ct, stored(raw[order], "f32"), "f32", rr[order], q, scopes, 10)
    assert np.array_equal(d_rr, d_ct) and np.array_equal(order[r_ct], r_rr)
    ix_rr.close()
    ix_ct.close()


def test_lifecycle_upsert_overwrite_move_clear(Index):
    rng = np.random.default_rng(7)
    n, dim = 3000, 384
    raw = rng.standard_normal((n + 500, dim)).astype(np.float32)
    labels = np.zeros(n + 500, dtype=np.uint32)
    labels[:n] = rng.integers(0, 4, n)
    ix = build(Index, raw[:n], "bf16", labels[:n])
    q = rng.standard_normal((9, dim)).astype(np.float32)
    scopes = np.array([1, 2, 3, 0, 1, 2, 3, 5, 1], dtype=np.uint32)
    check(ix, stored(raw[:n], "bf16"), "bf16", labels[:n], q, scopes, 10)
    check(ix, stored(raw[:n], "bf16"), "bf16", labels[:n], q, scopes, 10)
    assert ix.stat("scope_builds") == 1
    # more rows into an existing scope (the row store grows: the labels grow with it, new slots at scope 0 until labelled)
    ix.upsert(np.arange(n, n + 500, dtype=np.int64), raw[n:])
    check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert ix.stat("scope_builds") == 2
    labels[n:] = 2
    ix.set_scopes(np.arange(n, n + 500, dtype=np.int64), labels[n:])
    check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert ix.stat("scope_builds") == 3
    # a vector overwritten keeps its scope
    slot = int(np.flatnonzero(labels == 3)[0])
    raw[slot] = q[2]
    ix.upsert(np.array([slot], dtype=np.int64), raw[slot : slot + 1])
    _, rows = check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert rows[2, 0] == slot
    # a slot moved to another scope (listed twice: the last label holds), to a new scope, and a scope cleared to 0
    labels[slot] = 1
    ix.set_scopes(np.array([slot, 7, slot], dtype=np.int64), np.array([2, labels[7], 1], dtype=np.uint32))
    _, rows = check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert slot not in rows[2].tolist()
    labels[[3, 4]] = 5
    ix.set_scopes(np.array([4, 3], dtype=np.int64), np.array([5, 5], dtype=np.uint32))
    _, rows = check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert sorted(rows[7, :2].tolist()) == [3, 4] and ix.stat("scopes") == 5
    gone = np.flatnonzero(labels == 2)
    labels[gone] = 0
    ix.set_scopes(gone.astype(np.int64), np.zeros(gone.size, dtype=np.uint32))
    _, rows = check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert (rows[1] == -1).all()
    # bad arguments change nothing
    before = ix.stat("scope_builds")
    with pytest.raises(native.NativeLibraryError):
        ix.set_scopes(np.array([0], dtype=np.int64), np.array([native.MAX_SCOPE + 1], dtype=np.uint32))
    with pytest.raises(native.NativeLibraryError):
        ix.set_scopes(np.array([ix.count()], dtype=np.int64), np.array([1], dtype=np.uint32))
    check(ix, stored(raw, "bf16"), "bf16", labels, q, scopes, 10)
    assert ix.stat("scope_builds") == before
    ix.close()


def test_an_index_that_never_saw_a_scope(Index):
    rng = np.random.default_rng(8)
    raw = rng.standard_normal((2000, 256)).astype(np.float32)
    ix = Index(256, dtype="f16")
    q = rng.standard_normal((3, 256)).astype(np.float32)
    dist, rows = ix.search_scoped(q, np.array([0, 1, 0], dtype=np.uint32), 5)          # nothing stored
    assert (rows == -1).all() and np.isinf(dist).all()
    ix.upsert(np.arange(2000, dtype=np.int64), raw)
    dist, rows = check(ix, stored(raw, "f16"), "f16", np.zeros(2000, dtype=np.uint32), q, np.array([0, 1, 0], dtype=np.uint32), 5)
    d_all, r_all = ix.search(q, 5)
    assert np.array_equal(rows[[0, 2]], r_all[[0, 2]]) and np.array_equal(dist[[0, 2]], d_all[[0, 2]])
    ix.close()


def test_scoped_keys_of_two_shards_merge_to_the_oracle_answer(Index):
    from codd_query_engine_amd.knn_index import merge_keys

    import torch

    rng = np.random.default_rng(9)
    n, dim, cut, k = 9000, 384, 5000, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    labels = rng.integers(0, 5, n).astype(np.uint32)
    raw[cut + 11] = raw[17]
    labels[17] = labels[cut + 11] = 3                                     # one vector on both shards, one scope: the lower global row first
    a, b = build(Index, raw[:cut], "f32", labels[:cut]), build(Index, raw[cut:], "f32", labels[cut:])
    q = rng.standard_normal((7, dim)).astype(np.float32)
    q[0] = raw[17]
    scopes = np.array([3, 1, 2, 0, 4, 77, 3], dtype=np.uint32)
    keys = torch.cat([a.search_keys_scoped(q, scopes, k, 0), b.search_keys_scoped(q, scopes, k, cut)], dim=1)
    _, dist, rows = merge_keys(keys, k)
    d_ref, r_ref = scoped_reference(stored(raw, "f32"), "f32", labels, o.normalize_rows(q), scopes, k)
    assert np.array_equal(rows.cpu().numpy(), r_ref) and np.array_equal(dist.cpu().numpy(), d_ref)
    assert r_ref[0, 0] == 17 and r_ref[0, 1] == cut + 11
    a.close()
    b.close()


def test_a_million_rows_hundred_scopes_batch_of_256(Index):
    """The grid of a real batch: 256 queries over 100 scopes of 1M x 768 rows, and a single query whose list is cut into the most
    parts; 16 sampled queries (and the single one) against the oracle."""
    rng = np.random.default_rng(10)
    n, dim, ns, k = 1_000_000, 768, 100, 10
    ix = Index(dim, dtype="f32")
    ix.reserve(n)
    raw = np.empty((n, dim), dtype=np.float32)
    for lo in range(0, n, 100_000):
        raw[lo : lo + 100_000] = rng.standard_normal((100_000, dim), dtype=np.float32)
        ix.upsert(np.arange(lo, lo + 100_000, dtype=np.int64), raw[lo : lo + 100_000])
    labels = (rng.integers(0, ns, n) + 1).astype(np.uint32)
    labels[rng.integers(0, n, 1000)] = 0
    ix.set_scopes(np.arange(n, dtype=np.int64), labels)
    q = rng.standard_normal((256, dim)).astype(np.float32)
    scopes = (rng.integers(0, ns, 256) + 1).astype(np.uint32)
    scopes[:8] = 42                                                      # two full work items of one scope
    dist, rows = ix.search_scoped(q, scopes, k)
    sample = [0, 5, 7, 8] + rng.choice(np.arange(9, 256), 12, replace=False).tolist()
    for b in sample:
        members = np.flatnonzero(labels == scopes[b])
        d, i = o.search(o.normalize_rows(raw[members]), "f32", o.normalize_rows(q[b : b + 1]), k)
        assert np.array_equal(rows[b], members[i[0]]) and np.array_equal(dist[b], d[0]), b
    d1, r1 = ix.search_scoped(q[5:6], scopes[5:6], 100)
    members = np.flatnonzero(labels == scopes[5])
    d, i = o.search(o.normalize_rows(raw[members]), "f32", o.normalize_rows(q[5:6]), 100)
    assert np.array_equal(r1[0], members[i[0]]) and np.array_equal(d1[0], d[0])
    assert ix.stat("scope_builds") == 1 and ix.stat("scopes") == ns
    ix.close()


def test_facade_and_store_on_the_hip_engine_persist_and_reload(tmp_path):
    from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore

    client = KnnClient(device="cuda:0", path=str(tmp_path))
    store = MetricsSemanticMetadataStore(client, collection_name="scoped")
    spaces = ["prod:api", "staging:api", "prod:billing"]
    for ns in spaces:
        for i in range(40):
            store.index_metadata(ns, {"metric_name": f"http_request_duration_seconds_{i}", "description": f"HTTP request latency of route {i}",
                                      "category": "application", "golden_signal_type": "latency"})
    store.index_metadata("prod:billing", {"metric_name": "invoice_latency_seconds", "description": "Invoice rendering latency", "category": "application"})
    col = client.get_collection("scoped")
    out = col.query(query_texts=["high latency"], n_results=10, where={"namespace": "staging:api"})
    assert len(out["ids"][0]) == 10 and all(i.startswith("staging:api#") for i in out["ids"][0])
    everything = col.query(query_texts=["high latency"], n_results=121)
    want = [i for i in everything["ids"][0] if i.startswith("staging:api#")][:10]   # the scoped answer is the global order, filtered
    want_d = [d for i, d in zip(everything["ids"][0], everything["distances"][0]) if i.startswith("staging:api#")][:10]
    assert out["ids"][0] == want and out["distances"][0] == want_d
    hits = store.search_metadata("invoice latency", n_results=100, namespace="prod:billing")
    assert len(hits) == 41 and {h["namespace"] for h in hits} == {"prod:billing"}
    assert "invoice_latency_seconds" in [h["metric_name"] for h in hits]
    assert store.search_metadata("invoice latency", namespace="nobody") == []
    mixed = col.query(query_texts=["high latency", "high latency"], n_results=10, where=[None, {"namespace": {"$eq": "prod:api"}}])
    assert mixed["ids"][0] == everything["ids"][0][:10] and all(i.startswith("prod:api#") for i in mixed["ids"][1])
    got = MetricsSearchClient(store).search_relevant_metrics("high latency", limit=5, namespace="prod:api")
    assert len(got) == 5
    assert client.persist() == 1
    fresh = KnnClient(device="cuda:0", path=str(tmp_path))
    again = fresh.get_collection("scoped")
    assert again.query(query_texts=["high latency"], n_results=10, where={"namespace": "staging:api"}) == out
    assert MetricsSemanticMetadataStore(fresh, collection_name="scoped").search_metadata("invoice latency", n_results=100, namespace="prod:billing") == hits
