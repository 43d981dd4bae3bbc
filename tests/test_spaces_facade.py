"""l2 and ip collections through the façade, host logic on the checker engine (tests/_space_oracle_engine.py):
ChromaDB's distances against a numpy brute force, `where` / `where_document` / delete / compact as for cosine, the space kept by
a persistence round trip, and a reload under another space refused."""

import json

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient
from tests import _space_oracle_engine as soe
from tests._oracle_engine import OracleEngine

D, N = 24, 60


def data(seed=3):
    rng = np.random.default_rng(seed)
    vecs = (rng.standard_normal((N, D)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    q = (1.3 * rng.standard_normal((4, D))).astype(np.float32)
    metas = [{"namespace": "a" if i % 3 else "b", "rank": i, "kind": "even" if i % 2 == 0 else "odd"} for i in range(N)]
    docs = [f"document {i} " + ("alpha" if i % 4 == 0 else "beta") for i in range(N)]
    return vecs, q, metas, docs


def brute(space, vecs, q, member):
    """(ids, fp64 distances) of one query among the records `member` names, by ChromaDB's definitions"""
    v, x = vecs.astype(np.float64), q.astype(np.float64)
    dist = ((x[None, :] - v) ** 2).sum(axis=1) if space == "l2" else 1.0 - v @ x
    order = [i for i in np.lexsort((np.arange(N), dist)) if member[i]]
    return order, dist


def fill(space, made=None, path=None):
    client = KnnClient(engine_factory=soe.factory("f32", made), path=path)
    col = client.get_or_create_collection("c", metadata={"hnsw:space": space})
    vecs, q, metas, docs = data()
    col.upsert(ids=[f"id{i}" for i in range(N)], embeddings=vecs, metadatas=metas, documents=docs)
    return client, col, vecs, q


def check(space, res, vecs, q, member, k):
    for b in range(q.shape[0]):
        order, dist = brute(space, vecs, q[b], member)
        want = order[:k]
        assert res["ids"][b] == [f"id{i}" for i in want], (space, b)
        got = np.array(res["distances"][b])
        scale = np.abs(q[b]).sum() * np.abs(vecs).max() + 1.0
        assert np.allclose(got, dist[want], rtol=1e-5, atol=1e-5 * scale), (space, b, got, dist[want])


@pytest.mark.parametrize("space", ["l2", "ip"])
def test_query_returns_chromadb_distances_of_the_space(space):
    made = []
    _, col, vecs, q = fill(space, made)
    assert col.space == space and made[0].space == space
    assert made[0].normalize_args == [False], "a non-cosine collection stores its embeddings as given"
    check(space, col.query(query_embeddings=q, n_results=7), vecs, q, np.ones(N, bool), 7)
    if space == "l2":
        own = col.query(query_embeddings=vecs[11:12], n_results=1)
        assert own["ids"][0] == ["id11"] and own["distances"][0] == [0.0]


@pytest.mark.parametrize("space", ["l2", "ip"])
def test_where_where_document_delete_and_compact_behave_as_for_cosine(space):
    made = []
    _, col, vecs, q = fill(space, made)
    ns_a = np.array([i % 3 != 0 for i in range(N)])
    check(space, col.query(query_embeddings=q, n_results=5, where={"namespace": "a"}), vecs, q, ns_a, 5)
    assert made[0].calls[-1] == "search_scoped"
    general = np.array([i >= 20 and i % 2 == 0 for i in range(N)])
    check(space, col.query(query_embeddings=q, n_results=5, where={"$and": [{"rank": {"$gte": 20}}, {"kind": "even"}]}), vecs, q, general, 5)
    assert made[0].calls[-1] == "search_masked"
    alpha = np.array([i % 4 == 0 for i in range(N)])
    check(space, col.query(query_embeddings=q, n_results=5, where_document={"$contains": "alpha"}), vecs, q, alpha, 5)
    assert col.query(query_embeddings=q, n_results=5, where={"namespace": "nobody"})["ids"] == [[] for _ in range(4)]
    # delete, then the same answers without the deleted records; compact renumbers the slots and changes nothing a caller sees
    gone = [0, 4, 8, 21, 22]
    col.delete(ids=[f"id{i}" for i in gone])
    live = np.ones(N, bool)
    live[gone] = False
    check(space, col.query(query_embeddings=q, n_results=9), vecs, q, live, 9)
    check(space, col.query(query_embeddings=q, n_results=5, where_document={"$contains": "alpha"}), vecs, q, alpha & live, 5)
    before = col.query(query_embeddings=q, n_results=9)
    assert col.compact() == N - len(gone) and made[0].count() == N - len(gone)
    assert col.query(query_embeddings=q, n_results=9) == before
    check(space, col.query(query_embeddings=q, n_results=5, where={"namespace": "a"}), vecs, q, ns_a & live, 5)


@pytest.mark.parametrize("space", ["l2", "ip"])
def test_persistence_keeps_the_space_and_the_rows(space, tmp_path):
    writer, col, vecs, q = fill(space, path=str(tmp_path))
    before = col.query(query_embeddings=q, n_results=6)
    rows_before = col._engine.read_rows()
    assert writer.persist() == 1
    man = json.loads((tmp_path / "c" / "gen-00000001" / "manifest.json").read_text())
    assert man["metadata"]["hnsw:space"] == space
    made = []
    reader = KnnClient(engine_factory=soe.factory("f32", made), path=str(tmp_path))
    rcol = reader.get_or_create_collection("c")
    assert rcol.space == space and made[0].space == space
    assert np.array_equal(rcol._engine.read_rows(), rows_before), "rows of a non-cosine index persist and load bit for bit"
    assert rcol.query(query_embeddings=q, n_results=6) == before
    # an update published by the writer is picked up under the same space
    col.upsert(ids=["late"], embeddings=q[:1])
    assert writer.persist() == 1 and reader.reload() == 1
    assert rcol._engine.space == space
    top = rcol.query(query_embeddings=q[:1], n_results=1)
    assert top["ids"][0] == (["late"] if space == "l2" else col.query(query_embeddings=q[:1], n_results=1)["ids"][0])


def test_a_generation_of_another_space_is_refused_like_another_dtype(tmp_path):
    writer, _, _, q = fill("l2", path=str(tmp_path))
    other = KnnClient(engine_factory=soe.factory(), path=str(tmp_path))       # nothing on disk yet: "c" is its own, cosine
    mine = other.get_or_create_collection("c")
    mine.upsert(ids=["x"], embeddings=q[:1])
    assert mine.space == "cosine"
    writer.persist()
    with pytest.raises(ValueError, match="space"):
        other.reload()


def test_a_factory_lists_the_spaces_it_builds():
    bare = KnnClient(engine_factory=lambda dim: OracleEngine(dim))
    for space in ("l2", "ip"):
        with pytest.raises(ValueError):
            bare.get_or_create_collection(space, metadata={"hnsw:space": space})
    assert bare.get_or_create_collection("plain").space == "cosine"
    full = KnnClient(engine_factory=soe.factory())
    with pytest.raises(ValueError):
        full.get_or_create_collection("m", metadata={"hnsw:space": "manhattan"})
    assert full.get_or_create_collection("d").space == "cosine", "the default space stays cosine"
    # the default factory of a product client carries all three and passes the space on (no engine is built before the first upsert)
    product = KnnClient()
    assert product._engine_factory.spaces == ("cosine", "l2", "ip")
    assert product.get_or_create_collection("p", metadata={"hnsw:space": "ip"}).space == "ip"


def test_a_stored_space_the_factory_cannot_build_is_an_error(tmp_path):
    writer, _, _, _ = fill("ip", path=str(tmp_path))
    writer.persist()
    with pytest.raises(ValueError, match="hnsw:space"):
        KnnClient(engine_factory=lambda dim: OracleEngine(dim), path=str(tmp_path))
