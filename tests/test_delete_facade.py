"""Collection.delete / compact above the engine, on a checker engine with tombstones (tests/_deleting_oracle_engine.py): what the
chromadb-shaped façade answers after records were deleted by id, by namespace and by both; the tie rule across a delete and a
re-insertion; compaction (explicit, automatic, at persist()) and the on-disk generation it leaves.  No GPU."""

import json
import os

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient
from oracle import knn_oracle as o
from tests._deleting_oracle_engine import DeletingOracleEngine
from tests._scoped_oracle_engine import ScopedOracleEngine

NAMESPACES = ["prod:api", "staging:api", "prod:billing"]
DIM = 48


def deleting_client(**kw):
    return KnnClient(engine_factory=lambda dim: DeletingOracleEngine(dim), **kw)


def fill(col, n=60, seed=3):
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    ns = [None if i % 5 == 4 else NAMESPACES[i % 3] for i in range(n)]
    md = [None if i % 10 == 9 else ({"k": i} if ns[i] is None else {"k": i, "namespace": ns[i]}) for i in range(n)]
    col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=md, documents=[f"doc {i}" for i in range(n)])
    return vecs, ns


def brute(vecs_by_id: dict, order: list, q, k):
    """Oracle over the records of `order` (insertion order = tie order): (ids, distances) of one query."""
    if not order:
        return [], []
    mat = np.stack([vecs_by_id[i] for i in order])
    d, i = o.search(o.normalize_rows(mat), "f32", o.normalize_rows(q[None, :]), min(k, len(order)))
    hit = i[0] >= 0
    return [order[j] for j in i[0][hit]], d[0][hit].tolist()


def test_delete_by_ids_is_reflected_by_count_get_and_query_and_unknown_ids_are_ignored():
    col = deleting_client().get_or_create_collection("c")
    vecs, _ = fill(col)
    by_id = {f"id{i}": vecs[i] for i in range(60)}
    q = np.random.default_rng(1).standard_normal(DIM).astype(np.float32)
    best = col.query(query_embeddings=q, n_results=5)["ids"][0]
    gone = [best[0], best[2], "id17", "never-stored"]
    col.delete(ids=gone)
    assert col.count() == 57
    assert col.get(ids=gone)["ids"] == []
    assert "id17" not in col.get()["ids"] and len(col.get()["ids"]) == 57
    assert col.get(limit=3, offset=0)["ids"] == [i for i in (f"id{j}" for j in range(60)) if i not in gone][:3]
    order = [f"id{i}" for i in range(60) if f"id{i}" not in gone]
    out = col.query(query_embeddings=q, n_results=5)
    ids, dists = brute(by_id, order, q, 5)
    assert out["ids"] == [ids] and out["distances"] == [dists]
    assert out["documents"][0] == [f"doc {int(i[2:])}" for i in ids]
    col.delete(ids=gone)  # a second time: nothing left to do
    col.delete(ids=["never-stored"])
    assert col.count() == 57


def test_delete_by_namespace_and_by_both():
    col = deleting_client().get_or_create_collection("c")
    vecs, ns = fill(col)
    q = np.random.default_rng(2).standard_normal(DIM).astype(np.float32)
    col.delete(where={"namespace": {"$eq": "staging:api"}})
    staging = [f"id{i}" for i, x in enumerate(ns) if x == "staging:api" and i % 10 != 9]
    assert staging and col.get(ids=staging)["ids"] == []
    assert col.count() == 60 - len(staging)
    assert col.query(query_embeddings=q, n_results=9, where={"namespace": "staging:api"})["ids"] == [[]]
    # both: only those of the ids that carry the namespace
    billing = [f"id{i}" for i, x in enumerate(ns) if x == "prod:billing" and i % 10 != 9]
    api = [f"id{i}" for i, x in enumerate(ns) if x == "prod:api" and i % 10 != 9]
    before = col.count()
    col.delete(ids=[billing[0], billing[1], api[0], "nobody"], where={"namespace": "prod:billing"})
    assert col.count() == before - 2
    assert col.get(ids=[billing[0], billing[1], api[0]])["ids"] == [api[0]]
    scoped = col.query(query_embeddings=q, n_results=100, where={"namespace": "prod:billing"})["ids"][0]
    assert sorted(scoped) == sorted(billing[2:])
    # a namespace nobody stored: nothing happens
    col.delete(where={"namespace": "nobody"})
    assert col.count() == before - 2


def test_delete_needs_ids_or_where_and_rejects_other_filters():
    col = deleting_client().get_or_create_collection("c")
    fill(col)
    with pytest.raises(ValueError, match="ids"):
        col.delete()
    for bad in ({"category": "x"}, {"namespace": {"$in": ["a"]}}, [{"namespace": "prod:api"}]):
        with pytest.raises(ValueError, match="namespace"):
            col.delete(where=bad)
    assert col.count() == 60


def test_reupsert_of_a_deleted_id_is_a_new_insertion_and_n_results_is_clamped_to_the_live_count():
    col = deleting_client().get_or_create_collection("c")
    vecs, _ = fill(col, n=12)
    eng = col._engine
    col.delete(ids=["id3", "id4"])
    fresh = np.random.default_rng(8).standard_normal((1, DIM)).astype(np.float32)
    col.upsert(ids=["id3"], embeddings=fresh, metadatas=[{"namespace": "prod:api"}], documents=["again"])
    assert col._slot_of["id3"] == 12 and eng.count() == 13 and eng.live_count() == 11 and col.count() == 11
    assert col.get(ids=["id3"])["documents"] == ["again"]
    q = np.random.default_rng(4).standard_normal(DIM).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=50)
    by_id = {f"id{i}": vecs[i] for i in range(12)}
    by_id["id3"] = fresh[0]
    order = [f"id{i}" for i in range(12) if i not in (3, 4)] + ["id3"]
    ids, dists = brute(by_id, order, q, 50)
    assert len(ids) == 11 and out["ids"] == [ids] and out["distances"] == [dists]


def test_tie_goes_to_the_earlier_insertion_also_after_delete_and_readd():
    col = deleting_client().get_or_create_collection("c")
    rng = np.random.default_rng(6)
    twin = rng.standard_normal(DIM).astype(np.float32)
    others = rng.standard_normal((6, DIM)).astype(np.float32)
    col.upsert(ids=["early", "late"] + [f"o{i}" for i in range(6)], embeddings=np.vstack([twin, twin, others]))
    assert col.query(query_embeddings=twin, n_results=2)["ids"] == [["early", "late"]]
    col.delete(ids=["early"])
    assert col.query(query_embeddings=twin, n_results=2)["ids"][0][0] == "late"
    col.upsert(ids=["early"], embeddings=twin[None, :])  # the same vector again: now the LATER insertion
    out = col.query(query_embeddings=twin, n_results=2)
    assert out["ids"] == [["late", "early"]] and out["distances"][0][0] == out["distances"][0][1]
    col.compact()
    assert col.query(query_embeddings=twin, n_results=2)["ids"] == [["late", "early"]]


def test_compact_keeps_every_answer_and_renumbers_the_host_lists():
    col = deleting_client().get_or_create_collection("c")
    fill(col)
    eng = col._engine
    col.delete(ids=[f"id{i}" for i in range(0, 60, 3)])
    q = np.random.default_rng(12).standard_normal((5, DIM)).astype(np.float32)
    where = [None, {"namespace": "prod:api"}, {"namespace": "staging:api"}, None, {"namespace": "prod:billing"}]
    before_plain, before_scoped, before_get = col.query(query_embeddings=q, n_results=8), col.query(query_embeddings=q, n_results=8, where=where), col.get()
    assert eng.count() == 60 and eng.compactions == 0
    assert col.compact() == 40
    assert eng.count() == 40 and eng.live_count() == 40 and eng.compactions == 1 and len(col._ids) == 40
    assert col.query(query_embeddings=q, n_results=8) == before_plain
    assert col.query(query_embeddings=q, n_results=8, where=where) == before_scoped
    assert col.get() == before_get
    assert all(col._ids[s] == i for i, s in col._slot_of.items())
    assert col.compact() == 40 and eng.compactions == 1  # nothing dead: nothing to do
    col.upsert(ids=["new"], embeddings=q[:1])  # the next insertion takes the slot behind the live rows
    assert col._slot_of["new"] == 40


def test_auto_compaction_fires_once_dead_slots_exceed_half_of_all_slots():
    col = deleting_client().get_or_create_collection("c")
    fill(col, n=20)
    eng = col._engine
    col.delete(ids=[f"id{i}" for i in range(10)])  # exactly half: not yet
    assert eng.compactions == 0 and eng.count() == 20 and col.count() == 10
    col.delete(ids=["id10"])  # 11 of 20
    assert eng.compactions == 1 and eng.count() == 9 and col.count() == 9 and len(col._ids) == 9
    assert col.get()["ids"] == [f"id{i}" for i in range(11, 20)]


def test_persist_writes_a_compact_generation_and_a_fresh_client_answers_the_same(tmp_path):
    client = deleting_client(path=str(tmp_path))
    col = client.get_or_create_collection("c")
    fill(col)
    col.delete(ids=[f"id{i}" for i in range(5, 25)])
    q = np.random.default_rng(13).standard_normal((3, DIM)).astype(np.float32)
    where = [{"namespace": "prod:api"}, None, {"namespace": "staging:api"}]
    want_plain, want_scoped = col.query(query_embeddings=q, n_results=6), col.query(query_embeddings=q, n_results=6, where=where)
    assert client.persist() == 1
    assert col._engine.count() == 40  # persist() compacted
    gen = open(os.path.join(tmp_path, "c", "CURRENT")).read().strip()
    manifest = json.load(open(os.path.join(tmp_path, "c", gen, "manifest.json")))
    assert manifest["count"] == 40 and manifest["format_version"] == 1
    assert os.path.getsize(os.path.join(tmp_path, "c", gen, "rows.bin")) == 40 * manifest["padded_dim"] * 4
    ids = json.load(open(os.path.join(tmp_path, "c", gen, "ids.json")))
    assert len(ids) == 40 and None not in ids
    other = deleting_client(path=str(tmp_path))
    col2 = other.get_collection("c")
    assert col2.count() == 40
    assert col2.query(query_embeddings=q, n_results=6) == want_plain
    assert col2.query(query_embeddings=q, n_results=6, where=where) == want_scoped
    # a reader that was already open picks the generation up with reload()
    col.delete(where={"namespace": "prod:billing"})
    want = col.query(query_embeddings=q, n_results=6)
    assert client.persist() == 1 and other.reload() == 1
    assert other.get_collection("c").query(query_embeddings=q, n_results=6) == want


def test_deleting_everything_leaves_an_empty_collection_that_persists_and_fills_again(tmp_path):
    client = deleting_client(path=str(tmp_path))
    col = client.get_or_create_collection("c")
    vecs, _ = fill(col, n=8)
    col.delete(ids=[f"id{i}" for i in range(8)])
    assert col.count() == 0 and col.get()["ids"] == []
    assert col.query(query_embeddings=vecs[:2], n_results=3)["ids"] == [[], []]
    client.persist()
    assert deleting_client(path=str(tmp_path)).get_collection("c").count() == 0
    col.upsert(ids=["a"], embeddings=vecs[:1])
    assert col.count() == 1 and col.query(query_embeddings=vecs[:1], n_results=3)["ids"] == [["a"]]


def test_an_engine_without_delete_raises_not_implemented():
    col = KnnClient(engine_factory=lambda dim: ScopedOracleEngine(dim)).get_or_create_collection("c")
    fill(col, n=10)
    with pytest.raises(NotImplementedError, match="delete"):
        col.delete(ids=["id1"])
    with pytest.raises(NotImplementedError, match="delete"):
        col.delete(where={"namespace": "prod:api"})
    assert col.count() == 10 and col.get(ids=["id1"])["ids"] == ["id1"]
