"""Metadata filters on the GPU, through the C ABI and its bindings (codd_knn_set_column_host / codd_knn_eval_where).
The expected words of every filter are the packed host mask of Collection._eval_where — the host route, which exists without any
of this — on a twin collection over the checker engine, word for word, the bits at and above the count included.  dim = 8."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from codd_query_engine_amd import where_columns as wc
from tests import _where_cases as cases

pytestmark = pytest.mark.gpu

COUNTS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049]


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


class Pair:
    """A device index with its columns, and the host collection (checker engine) that says what every filter means.  Every write
    goes to both; the columns are maintained the way the façade maintains them, through ColumnSet."""

    def __init__(self, Index, n, seed, deleted=0):
        self.ref, vecs, _ = cases.random_collection(n, seed)
        self.ix = Index(cases.DIM)
        self.ix.upsert(np.arange(n, dtype=np.int64), vecs)
        self.cs = wc.ColumnSet()
        self.rng = np.random.default_rng(seed + 1000)
        if deleted:
            self.delete([f"id{int(i)}" for i in self.rng.choice(n, size=deleted, replace=False)])

    def upsert(self, ids, metadatas):
        vecs = self.rng.standard_normal((len(ids), cases.DIM)).astype(np.float32)
        self.ref.upsert(ids=ids, embeddings=vecs, metadatas=metadatas)
        slots = np.array([self.ref._slot_of[i] for i in ids], dtype=np.int64)
        self.ix.upsert(slots, vecs)
        self.cs.resize(len(self.ref._ids))
        if metadatas is not None:
            for col, tags, cells in self.cs.encode_slots(metadatas):
                self.ix.set_column(col.index, slots, tags, cells)
                self.cs.wrote(col, slots, tags, cells)

    def delete(self, ids):
        slots = np.array([self.ref._slot_of[i] for i in ids], dtype=np.int64)
        n = len(self.ref._ids)
        self.ref.delete(ids=ids)
        assert len(self.ref._ids) == n, "the helper must stay under the façade's auto-compaction share"
        self.ix.delete(slots)

    def compact(self):
        keep = [s for s, doc_id in enumerate(self.ref._ids) if doc_id is not None]
        assert self.ref.compact() == self.ix.compact() == len(keep)
        self.cs.compacted(keep)

    def program(self, where):
        self.ref._check_where(where)
        for key in wc.filter_keys(where):
            if self.cs.get(key) is None:
                col = self.cs.build(key, self.ref._metadatas)
                assert not col.host_only, key
                self.ix.set_column(col.index, None, col.tags, col.cells)
        prog = wc.compile_where(where, self.cs.by_key)
        assert prog is not None, where
        return prog

    def words(self, prog) -> np.ndarray:
        return self.ix.eval_where(prog).cpu().numpy().view(np.uint32)

    def check(self, where):
        assert self.ix.count() == len(self.ref._ids)
        before = self.ix.stat("where_evals")
        got, want = self.words(self.program(where)), cases.pack(self.ref._eval_where(where))
        assert self.ix.stat("where_evals") == before + 1
        assert got.shape == want.shape, (got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (where, bad[:4], [hex(int(got[w])) for w in bad[:4]], [hex(int(want[w])) for w in bad[:4]])
        return want


@pytest.fixture(scope="module", params=COUNTS)
def pair(Index, request):
    n = request.param
    p = Pair(Index, n, seed=100 + n, deleted=n // 5)
    yield p
    p.ix.close()


@pytest.mark.parametrize("where", cases.FILTERS, ids=lambda w: repr(w)[:50])
def test_every_operator_and_class_at_every_row_count(pair, where):
    pair.check(where)


def test_the_filters_say_something_at_the_largest_count(Index):
    p = Pair(Index, 2049, seed=100 + 2049, deleted=2049 // 5)
    counts = [int(p.ref._eval_where(w).sum()) for w in cases.FILTERS]
    assert 0 in counts and p.ref.count() in counts and sum(0 < c < p.ref.count() for c in counts) > 30
    p.ix.close()


@pytest.mark.parametrize("max_blocks", [1, 2, 3])
def test_a_count_that_needs_several_passes_of_the_grid(Index, max_blocks):
    """A workgroup step covers 1,024 rows and the grid is capped at eight workgroups per compute unit: millions of rows before a
    workgroup takes a second step.  "where_max_blocks" caps the grid for this test instead: 5,000 rows are five steps, taken by one,
    two (uneven) and three workgroups.  The answer never depends on the grid."""
    p = Pair(Index, 5000, seed=7, deleted=900)
    p.ix.set_option("where_max_blocks", max_blocks)
    for where in cases.FILTERS[::3]:
        p.check(where)
    p.ix.close()


def big_filters():
    leaves = [{"size": {"$gt": i - 16.5}} if i % 2 else {"weight": {"$lte": (i - 16) / 8}} for i in range(wc.MAX_LEAVES)]
    nested = leaves[0]
    for leaf in leaves[1:]:   # to the right: every leaf is on the stack before the first operator runs (32 entries)
        nested = {"$or" if len(str(leaf)) % 2 else "$and": [leaf, nested]}
    return {
        "32 leaves, 63 operators": {"$or": [{"$and": leaves[:16]}, {"$and": leaves[16:]}]},
        "32 leaves on the stack": nested,
        "256 literals in one $in": {"size": {"$in": [i / 2 for i in range(-128, 128)]}},
        "256 literals, negated, beside a second column": {"$and": [{"size": {"$nin": list(range(-100, 155))}}, {"color": {"$ne": "red"}}]},
        "leaves pushed twice (31 pushes of 16 leaves)": {"$and": [{"$or": leaves[:16]}, {"$or": leaves[1:16]}]},
    }


@pytest.mark.parametrize("name", list(big_filters()))
def test_programs_at_the_limits(Index, name):
    p = Pair(Index, 700, seed=3, deleted=100)
    where = big_filters()[name]
    prog = p.program(where)
    if name.startswith("32 leaves"):
        # the longest well-formed program: p pushes need p - 1 operators, so 63 of the 64 operator slots (one more is malformed, below)
        assert len(prog.leaves) == wc.MAX_LEAVES and len(prog.ops) == wc.MAX_OPS - 1
    if name.startswith("256"):
        assert len(prog.literals) == wc.MAX_LITERALS
    want = p.check(where)
    assert 0 < int(np.unpackbits(want.view(np.uint8)).sum()) < p.ref.count() or "stack" in name
    p.ix.close()


def test_write_sequences(Index):
    p = Pair(Index, 300, seed=5)
    filters = [{"color": {"$ne": "red"}}, {"size": {"$gt": 0}}, {"mixed": {"$in": [True, 1, "x"]}}, {"flag": {"$nin": [True]}},
               {"$and": [{"weight": {"$lte": 0.5}}, {"$or": [{"color": "teal"}, {"nobody": {"$ne": 3}}]}]}]
    all_ok = lambda: [p.check(w) for w in filters]  # noqa: E731
    all_ok()
    ncols = len(p.cs.device_columns())
    cap0 = p.ix.stat("capacity_rows")
    assert p.ix.stat("where_columns") == ncols and p.ix.stat("where_column_bytes") == 9 * cap0 * ncols
    # tombstones are honoured without any column write
    p.delete([f"id{i}" for i in range(40, 120, 3)])
    all_ok()
    # set_column on a subset of the slots: replaced metadata, keys that disappear, a record that loses its metadata
    p.upsert(["id3", "id4", "id5", "id6", "id299"], [{"color": "teal"}, {"size": 2.5, "flag": False}, None, {}, {"mixed": "x", "weight": -0.0}])
    all_ok()
    assert p.ref._eval_where({"color": "teal"})[3]
    # growth past the initial capacity: the columns grow with the rows, slots nobody wrote a cell for read absent
    rng = np.random.default_rng(9)
    p.upsert([f"more{i}" for i in range(900)], [cases.random_metadata(rng, i) for i in range(900)])
    p.upsert([f"bare{i}" for i in range(300)], None)
    cap1 = p.ix.stat("capacity_rows")
    assert cap1 > cap0 and p.ix.count() == 1500 and p.ix.stat("where_column_bytes") == 9 * cap1 * ncols
    all_ok()
    # compaction moves the columns with the rows; the vacated slots read absent again when rows are written there
    p.delete([f"more{i}" for i in range(0, 900, 2)] + [f"id{i}" for i in range(200, 260)])
    p.ix.set_option("compact_chunk_rows", 97)
    p.compact()
    assert p.ix.count() == p.ref.count() == len(p.ref._ids)
    all_ok()
    p.upsert([f"after{i}" for i in range(400)], None)
    all_ok()
    absent = p.ref._eval_where({"color": {"$ne": "no such color"}})
    assert absent[-400:].all()
    # a load replaces the rows: the columns are gone, and a program that names one is refused on the host
    prog = p.program(filters[0])
    rows = p.ix.read_rows()
    evals = p.ix.stat("where_evals")
    p.ix.load_rows(rows[:10], 0)
    assert p.ix.stat("where_columns") == 0 and p.ix.stat("where_column_bytes") == 0
    with pytest.raises(native.NativeLibraryError, match="code -22.*has not been set"):
        p.ix.eval_where(prog)
    assert p.ix.stat("where_evals") == evals
    p.ix.close()


def test_set_column_rules(Index):
    p = Pair(Index, 100, seed=6)
    tags, cells = np.ones(100, dtype=np.uint8), np.zeros(100, dtype=np.uint64)
    p.ix.set_column(0, None, tags, cells)
    p.ix.delete(np.array([7], dtype=np.int64))
    for bad in (lambda: p.ix.set_column(32, None, tags, cells), lambda: p.ix.set_column(-1, None, tags, cells),
                lambda: p.ix.set_column(0, None, np.ones(101, dtype=np.uint8), np.zeros(101, dtype=np.uint64)),
                lambda: p.ix.set_column(0, np.array([100]), tags[:1], cells[:1]), lambda: p.ix.set_column(0, np.array([-1]), tags[:1], cells[:1]),
                lambda: p.ix.set_column(0, np.array([7]), tags[:1], cells[:1]), lambda: p.ix.set_column(0, np.array([1]), np.array([4], dtype=np.uint8), cells[:1])):
        with pytest.raises(native.NativeLibraryError, match="code -22"):
            bad()
    # a slot listed more than once keeps the last value
    p.ix.set_column(0, np.array([5, 9, 5]), np.array([1, 1, 1], dtype=np.uint8), np.array([0, 0, 1], dtype=np.uint64))
    flag_is_true = type("P", (), {"leaves": [(0, wc.TAG_BOOL, wc.KIND_IN, 0, 0, 1)], "literals": [1], "ops": [0]})
    bits = np.unpackbits(p.ix.eval_where(flag_is_true).cpu().numpy().view(np.uint8), bitorder="little")[:100]
    assert np.flatnonzero(bits).tolist() == [5]
    p.ix.drop_columns()
    assert p.ix.stat("where_columns") == 0
    p.ix.close()


MALFORMED = {
    "an unset column": dict(leaves=[(5, 2, 0, 0, 0, 1)], literals=[0], ops=[0]),
    "a column outside the index": dict(leaves=[(32, 2, 0, 0, 0, 1)], literals=[0], ops=[0]),
    "a literal range past the literals": dict(leaves=[(0, 2, 0, 0, 1, 2)], literals=[0, 1], ops=[0]),
    "stack underflow": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[0, wc.OP_AND]),
    "an operator before any value": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[wc.OP_OR, 0]),
    "two values left": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[0, 0]),
    "64 operators (a well-formed program has an odd number)": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[0] + [0, wc.OP_AND] * 31 + [0]),
    "33 stack entries": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[0] * 33 + [wc.OP_AND] * 31),
    "a comparison on a str class": dict(leaves=[(0, 3, wc.KIND_GT, 0, 0, 1)], literals=[0], ops=[0]),
    "a comparison with two literals": dict(leaves=[(0, 2, wc.KIND_LT, 0, 0, 2)], literals=[0, 1], ops=[0]),
    "a push of a leaf the program does not have": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[1]),
    "an unknown kind": dict(leaves=[(0, 2, 5, 0, 0, 1)], literals=[0], ops=[0]),
    "the absent class": dict(leaves=[(0, 0, 0, 0, 0, 1)], literals=[0], ops=[0]),
    "no leaf": dict(leaves=[], literals=[], ops=[0]),
    "no operator": dict(leaves=[(0, 2, 0, 0, 0, 1)], literals=[0], ops=[]),
}


@pytest.fixture(scope="module")
def small(Index):
    p = Pair(Index, 70, seed=8)
    p.check({"size": {"$gt": 0}})   # column 0 is set
    yield p
    p.ix.close()


@pytest.mark.parametrize("name", list(MALFORMED))
def test_a_malformed_program_is_refused_on_the_host(small, name):
    prog = type("P", (), MALFORMED[name])
    before = small.ix.stat("where_evals")
    with pytest.raises(native.NativeLibraryError, match="code -22"):
        small.ix.eval_where(prog)
    assert native.last_error().startswith("eval_where:")
    assert small.ix.stat("where_evals") == before


def test_the_wrong_number_of_words_is_refused(small):
    import ctypes

    prog = native.where_program(small.program({"size": {"$gt": 0}}))
    before = small.ix.stat("where_evals")
    assert small.ix._lib.codd_knn_eval_where(small.ix._h, ctypes.byref(prog), None, 2, None) == -22
    assert small.ix._lib.codd_knn_eval_where(small.ix._h, ctypes.byref(prog), None, 3, None) == -22   # the right number, no buffer
    assert small.ix.stat("where_evals") == before
