"""`where=` on the device through Collection.query: twin collections over the same data on the real engine, one
opted in ("codd:device_where": 1, or KnnClient(device_where=True)) and one not.  Every query must return equal ids and bit-equal
distances on both; the engine's "where_evals" stat rises on the opted-in twin — the route ran, it did not fall back silently —
and stays 0 on the other.  dim = 8."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, native
from codd_query_engine_amd import where_columns as wc
from tests import _where_cases as cases

pytestmark = pytest.mark.gpu

N = 700
QUERIES = np.random.default_rng(31).standard_normal((5, cases.DIM)).astype(np.float32)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    return torch


def same_answers(a, b, where=None, where_document=None, queries=QUERIES, k=9):
    """Both collections' answers to one query call; asserts that they are equal (ids, distance bits) and returns the ids."""
    got = [c.query(query_embeddings=queries, n_results=k, where=where, where_document=where_document) for c in (a, b)]
    assert got[0]["ids"] == got[1]["ids"], (where, where_document)
    assert np.array_equal(np.asarray(sum(got[0]["distances"], []), dtype=np.float32).view(np.uint32),
                          np.asarray(sum(got[1]["distances"], []), dtype=np.float32).view(np.uint32)), (where, where_document)
    assert got[0]["metadatas"] == got[1]["metadatas"]
    return got[0]["ids"]


def evals(col) -> int:
    return col._engine.stat("where_evals")


@pytest.fixture(scope="module")
def twins(gpu):
    plain, _, _ = cases.random_collection(N, seed=41, client=KnnClient(), deleted=90, documents=True)
    device, _, _ = cases.random_collection(N, seed=41, client=KnnClient(), deleted=90, documents=True, metadata={"codd:device_where": 1})
    assert device.device_where and device._has_device_where() and not plain._has_device_where()
    yield plain, device
    for c in (plain, device):
        c._engine.close()


@pytest.mark.parametrize("where", cases.FILTERS, ids=lambda w: repr(w)[:50])
def test_a_general_filter_gives_the_same_answers_on_the_device_route(twins, where):
    plain, device = twins
    device._where_bits_cache.clear()
    before = evals(device)
    ids = same_answers(plain, device, where)
    live = int(plain._eval_where(where).sum())
    assert [len(i) for i in ids] == [min(9, live)] * len(QUERIES)   # (nobody matches: empty inner lists, no error)
    assert evals(device) == before + 1 and evals(plain) == 0
    assert plain._engine.stat("where_columns") == 0 and len(plain._columns) == 0
    # the bitmap is cached: the same filter again launches nothing
    same_answers(plain, device, where)
    assert evals(device) == before + 1


def test_where_and_where_document_together(twins):
    plain, device = twins
    device._where_bits_cache.clear()
    before, uploads = evals(device), []
    original = device._words_on_device
    device._words_on_device = lambda mask: uploads.append(1) or original(mask)
    try:
        for where, wd in (({"size": {"$gt": 0}}, {"$contains": "color=red"}), ({"color": {"$ne": "red"}}, {"$not_contains": "flag=True"}),
                          ({"$or": [{"flag": True}, {"mixed": 1}]}, {"$or": [{"$contains": "size=-"}, {"$contains": "#1"}]}),
                          ({"size": 99}, {"$contains": "color"}), ({"namespace": "ns0"}, {"$contains": "size"})):
            same_answers(plain, device, where, wd)
        # a list of filters, one per query: None, a namespace form, general ones
        per_query = [{"size": {"$lt": 1}}, None, {"namespace": "ns0"}, {"color": {"$in": ["red", "blue"]}}, {"size": {"$lt": 1}}]
        same_answers(plain, device, per_query, {"$contains": "="})
    finally:
        del device._words_on_device
    assert evals(device) == before + 7 and uploads == [], "no mask travels to the device on this route"
    assert evals(plain) == 0


def test_a_list_of_filters_one_per_query(twins):
    plain, device = twins
    device._where_bits_cache.clear()
    before, scoped = evals(device), device._engine.stat("scoped_searches")
    per_query = [{"size": {"$gte": 2}}, None, {"namespace": "ns0"}, {"size": {"$gte": 2}}, {"$and": [{"flag": True}, {"color": {"$gt": "b"}}]}]
    same_answers(plain, device, per_query)
    assert evals(device) == before + 2                                   # two distinct general filters
    assert device._engine.stat("scoped_searches") == scoped + 1          # the namespace form keeps going to search_scoped


def test_filters_the_device_cannot_take_fall_back_to_the_host_route(gpu):
    plain, _, _ = cases.random_collection(300, seed=43, client=KnnClient())
    device, _, _ = cases.random_collection(300, seed=43, client=KnnClient(device_where=True))
    same_answers(plain, device, {"size": {"$gt": 1}})
    assert evals(device) == 1
    over_a_limit = {"$or": [{"size": {"$gt": i / 4}} for i in range(wc.MAX_LEAVES + 1)]}
    for where in [over_a_limit, {"size": {"$in": list(range(wc.MAX_LITERALS + 1))}}] + cases.HOST_FILTERS:
        same_answers(plain, device, where)
        assert evals(device) == 1, where
    # a value without a cell retires its column: filters on that key take the host route, the other keys stay on the device
    for c in (plain, device):
        c.upsert(ids=["big"], embeddings=QUERIES[:1], metadatas=[{"size": 2**53 + 1, "color": "red"}])
    assert device._columns.get("size").host_only
    assert "big" in same_answers(plain, device, {"size": {"$gt": 2**53}}, k=3)[0]
    same_answers(plain, device, {"size": {"$gt": 1}})
    assert evals(device) == 1
    same_answers(plain, device, {"color": "red"})
    assert evals(device) == 2
    for c in (plain, device):
        c._engine.close()


def test_write_sequences_keep_the_columns_in_step(gpu, tmp_path):
    writers = [KnnClient(path=str(tmp_path / name), device_where=on) for name, on in (("plain", False), ("device", True))]
    plain, device = (cases.random_collection(500, seed=47, client=c, documents=True)[0] for c in writers)
    filters = [{"color": {"$nin": ["red", "teal"]}}, {"size": {"$lte": 0}}, {"mixed": {"$in": [True, 1, "x"]}}, {"flag": {"$ne": True}},
               {"$and": [{"weight": {"$gt": -0.5}}, {"$or": [{"color": "teal"}, {"nobody": {"$ne": 3}}]}]}]

    def all_same(a=plain, b=device):
        before = evals(b)
        for where in filters:
            same_answers(a, b, where)
        assert evals(b) == before + len(filters)   # (every write dropped the cached bitmaps; none fell back)

    all_same()
    built = device._engine.stat("where_columns")
    assert built == len(device._columns.device_columns()) == 6
    for c in (plain, device):   # replaced metadata, lost keys, no metadata, metadatas=None, new records with and without metadata
        c.upsert(ids=["id3", "id4", "id5", "id6"], embeddings=QUERIES[:4], metadatas=[{"color": "teal"}, {"size": 2.5, "flag": False}, None, {}])
        c.upsert(ids=["id7", "id8"], embeddings=QUERIES[:2])
        c.upsert(ids=[f"new{i}" for i in range(700)], embeddings=np.random.default_rng(49).standard_normal((700, cases.DIM)).astype(np.float32),
                 metadatas=[cases.random_metadata(np.random.default_rng(50 + i), i) for i in range(700)])   # (past the first capacity)
        c.upsert(ids=["bare0", "bare1"], embeddings=QUERIES[:2])
    all_same()
    for c in (plain, device):
        c.delete(ids=[f"id{i}" for i in range(20, 90)])
    all_same()
    assert device._engine.stat("compactions") == 0
    for c in (plain, device):   # more than half of the slots are dead: the collection compacts by itself
        c.delete(ids=[f"new{i}" for i in range(640)])
    assert device._engine.stat("compactions") == 1 and device._engine.stat("where_columns") == built
    all_same()
    # persist, then a reader that loads the generation: its columns are derived again, nothing of them is on disk
    for w in writers:
        assert w.persist() == 1
    readers = [KnnClient(path=w.path, device_where=w.device_where) for w in writers]
    plain_r, device_r = (r.get_collection("c") for r in readers)
    assert device_r._engine.stat("where_columns") == 0 and len(device_r._columns) == 0
    all_same(plain_r, device_r)
    same_answers(plain, device_r, filters[0])   # (the reader answers as the writer does)
    # the writer goes on, persists again, the reader reloads: the reader's columns are dropped with its old engine
    for c in (plain, device):
        c.upsert(ids=["late0", "late1"], embeddings=QUERIES[:2], metadatas=[{"color": "teal", "size": -1}, {"flag": False}])
    for w, r in zip(writers, readers):
        assert w.persist() == 1 and r.reload() == 1
    plain_r, device_r = (r.get_collection("c") for r in readers)
    assert len(device_r._columns) == 0 and device_r._engine.stat("where_columns") == 0
    all_same(plain_r, device_r)
    all_same(plain, device)


def test_eval_where_feeds_the_sharded_and_the_ivf_search(twins, gpu):
    """index.eval_where(program) goes straight into ShardedSearcher.search(allow=) and ivf.search_ivf(allow=): the same keys, rows
    and distances as the same call under the uploaded host mask."""
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.sharded import ShardedSearcher

    plain, device = twins
    where = {"$and": [{"size": {"$gt": -3}}, {"color": {"$ne": "green"}}]}
    same_answers(plain, device, where)   # (builds the columns)
    engine = device._engine
    program = wc.compile_where(where, device._columns.by_key)
    mask = device._eval_where(where)
    before = evals(device)
    bits = engine.eval_where(program)
    assert evals(device) == before + 1 and np.array_equal(bits.cpu().numpy().view(np.uint32), cases.pack(mask))
    searcher = ShardedSearcher(engine, row_base=1000)
    d_dev, r_dev = searcher.search(QUERIES, 9, allow=bits)
    d_host, r_host = searcher.search(QUERIES, 9, allow=mask)
    assert gpu.equal(r_dev, r_host) and gpu.equal(d_dev, d_host) and int(r_dev.min()) >= 1000
    assert mask[(r_dev - 1000).cpu().numpy().ravel()].all()
    # IVF: a collection nobody deleted from, under a layout installed by hand (eight lists around eight of its own rows)
    fresh, vecs, _ = cases.random_collection(600, seed=53, client=KnnClient(device_where=True))
    same_answers(fresh, fresh, where)
    engine, mask = fresh._engine, fresh._eval_where(where)
    unit = vecs / np.linalg.norm(vecs, axis=1, keepdims=True)
    assign = np.argmax(unit @ unit[:8].T, axis=1)
    sizes = np.bincount(assign, minlength=8)
    assert sizes.min() > 0
    perm = gpu.from_numpy(np.argsort(assign, kind="stable").astype(np.int64)).to(engine.device)
    offsets = gpu.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(engine.device)
    cent = gpu.from_numpy(np.ascontiguousarray(unit[:8])).to(engine.device)
    native.check(engine._lib.codd_knn_ivf_install(engine._h, cent.data_ptr(), 8, perm.data_ptr(), offsets.data_ptr(), None), "codd_knn_ivf_install")
    gpu.cuda.synchronize()
    program = wc.compile_where(where, fresh._columns.by_key)
    d_dev, r_dev = ivf.search_ivf(engine, QUERIES, 9, 3, allow=engine.eval_where(program))
    d_host, r_host = ivf.search_ivf(engine, QUERIES, 9, 3, allow=mask)
    assert gpu.equal(r_dev, r_host) and gpu.equal(d_dev, d_host)
    hit = r_dev.cpu().numpy().ravel()
    assert mask[hit[hit >= 0]].all() and (hit >= 0).any()
    engine.close()
