"""The host half of `where=` on the device (codd_query_engine_amd/where_columns.py): the order-preserving number
keys, the column encoding and its host_only rule, the program compiler with every limit at its bound and one past it, and two
agreements — a numpy interpreter of the compiled programs (tests/_where_cases.py) over the column mirrors equals
Collection._eval_where bit for bit on a randomised collection, and mirrors maintained incrementally through a write sequence equal
columns built from scratch.  No GPU, no engine with eval_where: the façade here only maintains mirrors."""

import sys

import numpy as np
import pytest

from codd_query_engine_amd import where_columns as wc
from tests import _where_cases as cases


# ---------------------------------------------------------------------------------------------- key encoding
SORTED_NUMBERS = [float("-inf"), -1.7976931348623157e308, -(2**53), -3, -2.5, -1, -2.2250738585072014e-308, -5e-324, 0.0, 5e-324,
                  2.2250738585072014e-308, 0.5, 1, 2, 2**53, 1.7976931348623157e308, float("inf")]


def test_number_keys_are_monotone_and_fit_64_bits():
    keys = [wc.number_key(v) for v in SORTED_NUMBERS]
    assert all(k is not None and 0 <= k < 1 << 64 for k in keys)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert [wc.key_number(k) for k in keys] == [float(v) for v in SORTED_NUMBERS]


def test_the_two_zeros_agree_and_an_int_equals_its_float():
    assert wc.number_key(-0.0) == wc.number_key(0.0) == wc.number_key(0)
    assert wc.number_key(1) == wc.number_key(1.0)
    assert wc.number_key(-(2**53)) == wc.number_key(float(-(2**53)))


def test_a_bool_and_an_int_land_in_different_classes():
    col = wc.Column("k", 0)
    assert col.encode({"k": True}) == (wc.TAG_BOOL, 1) and col.encode({"k": False}) == (wc.TAG_BOOL, 0)
    assert col.encode({"k": 1}) == (wc.TAG_NUMBER, wc.number_key(1))
    assert col.encode({"k": "1"}) == (wc.TAG_STR, 1) and col.encode({"k": "x"}) == (wc.TAG_STR, 2) and col.encode({"k": "1"}) == (wc.TAG_STR, 1)
    assert col.encode({"other": 1}) == (wc.TAG_ABSENT, 0) and col.encode(None) == (wc.TAG_ABSENT, 0)
    assert not col.host_only


@pytest.mark.parametrize("value", [float("nan"), 2**53 + 1, -(2**53) - 1, 10**400, None, [1], {"a": 1}], ids=repr)
def test_a_value_without_a_cell_makes_the_column_host_only(value):
    assert wc.value_tag(value) == wc.TAG_ABSENT or wc.number_key(value) is None
    cs = wc.ColumnSet()
    col = cs.build("k", [{"k": 1}, {"k": value}, None])
    assert col.host_only and cs.device_columns() == [] and cs.has_room()
    assert wc.compile_where({"k": {"$eq": 1}}, cs.by_key) is None
    # ... and so does a value that arrives with a later write
    cs = wc.ColumnSet()
    col = cs.build("k", [{"k": 1}, None])
    assert not col.host_only and wc.compile_where({"k": 1}, cs.by_key) is not None
    assert cs.encode_slots([{"k": value}]) == [] and col.host_only
    assert wc.compile_where({"k": 1}, cs.by_key) is None


def test_infinities_have_keys():
    cs = wc.ColumnSet()
    col = cs.build("k", [{"k": float("inf")}, {"k": float("-inf")}])
    assert not col.host_only and col.cells[1] < col.cells[0]


# ---------------------------------------------------------------------------------------------- program compilation
def columns_over(values_by_key):
    cs = wc.ColumnSet()
    n = max(len(v) for v in values_by_key.values())
    for key, values in values_by_key.items():
        cs.build(key, [{key: values[i]} if i < len(values) else None for i in range(n)])
    return cs


@pytest.fixture()
def cs():
    return columns_over({"s": ["b", "a", "c"], "n": [1, 2.5, -3], "b": [True, False]})


def one_leaf(cs, where):
    prog = wc.compile_where(where, cs.by_key)
    assert prog is not None and prog.ops == [0] and len(prog.leaves) == 1, (where, prog and (prog.leaves, prog.ops))
    column, tag, kind, negate, first, count = prog.leaves[0]
    return column, tag, kind, negate, prog.literals[first : first + count]


def test_equality_operators_on_every_class(cs):
    s, n, b = (cs.get(k).index for k in "snb")
    assert one_leaf(cs, {"s": "a"}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [2])
    assert one_leaf(cs, {"s": {"$ne": "c"}}) == (s, wc.TAG_STR, wc.KIND_IN, 1, [3])
    assert one_leaf(cs, {"s": {"$in": ["c", "b", "c"]}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [3, 1])
    assert one_leaf(cs, {"s": {"$nin": ["a"]}}) == (s, wc.TAG_STR, wc.KIND_IN, 1, [2])
    assert one_leaf(cs, {"n": 2.5}) == (n, wc.TAG_NUMBER, wc.KIND_IN, 0, [wc.number_key(2.5)])
    assert one_leaf(cs, {"n": {"$ne": 1}}) == (n, wc.TAG_NUMBER, wc.KIND_IN, 1, [wc.number_key(1.0)])
    assert one_leaf(cs, {"n": {"$in": [1, 1.0, 7]}}) == (n, wc.TAG_NUMBER, wc.KIND_IN, 0, [wc.number_key(1), wc.number_key(7)])
    assert one_leaf(cs, {"n": {"$nin": [-3]}}) == (n, wc.TAG_NUMBER, wc.KIND_IN, 1, [wc.number_key(-3)])
    assert one_leaf(cs, {"b": True}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [1])
    assert one_leaf(cs, {"b": {"$ne": False}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 1, [0])
    assert one_leaf(cs, {"b": {"$in": [False, True]}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [0, 1])
    assert one_leaf(cs, {"b": {"$nin": [True]}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 1, [1])
    # a literal of another class than the stored values: a leaf of the literal's class (it matches no row of this column)
    assert one_leaf(cs, {"s": 1}) == (s, wc.TAG_NUMBER, wc.KIND_IN, 0, [wc.number_key(1)])


def test_comparisons_on_every_class(cs):
    s, n, b = (cs.get(k).index for k in "snb")
    for op, kind in (("$lt", wc.KIND_LT), ("$lte", wc.KIND_LE), ("$gt", wc.KIND_GT), ("$gte", wc.KIND_GE)):
        assert one_leaf(cs, {"n": {op: 2}}) == (n, wc.TAG_NUMBER, kind, 0, [wc.number_key(2)])
    # a bool is compared here, over {False, True}; a str over the dictionary's entries (codes b=1 a=2 c=3)
    assert one_leaf(cs, {"b": {"$gt": False}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [1])
    assert one_leaf(cs, {"b": {"$gte": False}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [0, 1])
    assert one_leaf(cs, {"b": {"$lt": False}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [])
    assert one_leaf(cs, {"b": {"$lte": False}}) == (b, wc.TAG_BOOL, wc.KIND_IN, 0, [0])
    assert one_leaf(cs, {"s": {"$gt": "a"}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [1, 3])
    assert one_leaf(cs, {"s": {"$gte": "b"}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [1, 3])
    assert one_leaf(cs, {"s": {"$lt": "b"}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [2])
    assert one_leaf(cs, {"s": {"$lte": "0"}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [])


def test_an_unknown_str_contributes_no_literal(cs):
    s = cs.get("s").index
    assert one_leaf(cs, {"s": "zzz"}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [])          # constant false
    assert one_leaf(cs, {"s": {"$ne": "zzz"}}) == (s, wc.TAG_STR, wc.KIND_IN, 1, [])  # ... negated: everybody
    assert one_leaf(cs, {"s": {"$in": ["zzz", "a"]}}) == (s, wc.TAG_STR, wc.KIND_IN, 0, [2])
    assert "zzz" not in cs.get("s").codes, "compiling a filter must not grow the dictionary"


def test_a_list_of_several_classes_is_one_leaf_per_class(cs):
    prog = wc.compile_where({"s": {"$in": ["a", 1, True, "zzz"]}}, cs.by_key)
    assert [leaf[1:4] for leaf in prog.leaves] == [(t, wc.KIND_IN, 0) for t in (wc.TAG_BOOL, wc.TAG_NUMBER, wc.TAG_STR)]
    assert prog.ops == [0, 1, wc.OP_OR, 2, wc.OP_OR]
    prog = wc.compile_where({"s": {"$nin": ["a", 1]}}, cs.by_key)
    assert [leaf[1:4] for leaf in prog.leaves] == [(wc.TAG_NUMBER, wc.KIND_IN, 1), (wc.TAG_STR, wc.KIND_IN, 1)] and prog.ops == [0, 1, wc.OP_AND]


def test_and_or_are_postfix_and_equal_leaves_are_emitted_once(cs):
    a, b, c = {"s": "a"}, {"n": {"$gt": 1}}, {"b": True}
    prog = wc.compile_where({"$and": [a, {"$or": [b, c, a]}, b]}, cs.by_key)
    assert len(prog.leaves) == 3 and prog.ops == [0, 1, 2, wc.OP_OR, 0, wc.OP_OR, wc.OP_AND, 1, wc.OP_AND]
    assert prog.columns() == sorted(cs.get(k).index for k in "snb")


def test_filters_that_cannot_run_on_the_device(cs):
    for where in ({"n": float("nan")}, {"n": {"$gt": 2**53 + 1}}, {"n": {"$in": [1, 10**400]}}, {"unbuilt": 1},
                  {"$or": [{"s": "a"}, {"n": {"$lte": float("nan")}}]}):
        assert wc.compile_where(where, cs.by_key) is None, where
    assert wc.compile_where({"n": {"$gt": float("inf")}}, cs.by_key) is not None


def test_a_str_comparison_within_the_literal_budget_and_one_over_it():
    names = [f"s{i:04d}" for i in range(wc.MAX_LITERALS + 1)]
    cs = columns_over({"s": names})
    prog = wc.compile_where({"s": {"$lt": names[wc.MAX_LITERALS]}}, cs.by_key)     # accepts exactly MAX_LITERALS strings
    assert prog is not None and prog.leaves[0][5] == wc.MAX_LITERALS
    assert wc.compile_where({"s": {"$lte": names[wc.MAX_LITERALS]}}, cs.by_key) is None


def test_each_limit_at_its_bound_and_one_past_it():
    cs = columns_over({"n": [1]})
    leaf = lambda i: {"n": {"$gt": i}}  # noqa: E731
    # leaves: 32 distinct ones, and with them the longest well-formed program — p pushes need p - 1 operators, 63 <= MAX_OPS
    prog = wc.compile_where({"$or": [leaf(i) for i in range(wc.MAX_LEAVES)]}, cs.by_key)
    assert prog is not None and len(prog.leaves) == wc.MAX_LEAVES and len(prog.ops) == 2 * wc.MAX_LEAVES - 1 == wc.MAX_OPS - 1
    assert wc.compile_where({"$or": [leaf(i) for i in range(wc.MAX_LEAVES + 1)]}, cs.by_key) is None
    # operators: 33 pushes of 32 distinct leaves are 65 operators
    assert wc.compile_where({"$or": [leaf(i) for i in range(wc.MAX_LEAVES)] + [leaf(0)]}, cs.by_key) is None
    # literals
    prog = wc.compile_where({"n": {"$in": list(range(wc.MAX_LITERALS))}}, cs.by_key)
    assert prog is not None and len(prog.literals) == wc.MAX_LITERALS
    assert wc.compile_where({"n": {"$in": list(range(wc.MAX_LITERALS + 1))}}, cs.by_key) is None
    prog = wc.compile_where({"$and": [{"n": {"$in": list(range(200))}}, {"n": {"$nin": list(range(56))}}]}, cs.by_key)
    assert prog is not None and len(prog.literals) == wc.MAX_LITERALS
    assert wc.compile_where({"$and": [{"n": {"$in": list(range(200))}}, {"n": {"$nin": list(range(57))}}]}, cs.by_key) is None
    # the stack: a filter nested to the right keeps every leaf on it
    nested = leaf(0)
    for i in range(1, wc.MAX_STACK):
        nested = {"$and": [leaf(i), nested]}
    prog = wc.compile_where(nested, cs.by_key)
    assert prog is not None and prog.ops[: wc.MAX_STACK] == list(range(wc.MAX_STACK)) and prog.fits()
    # columns per index
    cs = wc.ColumnSet()
    for i in range(wc.MAX_COLUMNS):
        assert not cs.build(f"k{i}", [{f"k{i}": i}]).host_only
    assert sorted(c.index for c in cs.device_columns()) == list(range(wc.MAX_COLUMNS)) and not cs.has_room()
    assert wc.compile_where({"$and": [{f"k{i}": i} for i in range(wc.MAX_COLUMNS)]}, cs.by_key) is not None
    assert cs.build("one more", [{"one more": 1}]).host_only
    assert wc.compile_where({"one more": 1}, cs.by_key) is None


# ---------------------------------------------------------------------------------------------- interpreter agreement
@pytest.fixture(scope="module")
def collection():
    col, _, _ = cases.random_collection(2300, seed=11, deleted=300)
    assert None in col._ids and len(col._ids) == 2300
    return col


@pytest.mark.parametrize("where", cases.FILTERS, ids=lambda w: repr(w)[:60])
def test_the_interpreted_program_equals_the_host_route_bit_for_bit(collection, where):
    col = collection
    col._check_where(where)
    cs = cases.build_columns(col, wc.filter_keys(where))
    prog = wc.compile_where(where, cs.by_key)
    assert prog is not None
    got = cases.interpret(prog, {c.index: c for c in cs.device_columns()}, col._live_mask())
    want = col._eval_where(where)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_the_filters_cover_everybody_nobody_and_something_in_between(collection):
    counts = [int(collection._eval_where(w).sum()) for w in cases.FILTERS]
    live = collection.count()
    assert 0 in counts and live in counts and any(0 < c < live for c in counts)


@pytest.mark.parametrize("where", cases.HOST_FILTERS, ids=lambda w: repr(w)[:60])
def test_filters_for_the_host_route_compile_to_none(collection, where):
    collection._check_where(where)
    assert wc.compile_where(where, cases.build_columns(collection, wc.filter_keys(where)).by_key) is None


# ---------------------------------------------------------------------------------------------- incremental equals rebuilt
class ColumnEngine(cases.MaskedOracleEngine):
    """The checker engine with the column half of the device protocol: it records what the façade sends.  eval_where is never
    reached in this file (the test builds the columns through _where_bits' first half by hand)."""

    def __init__(self, dim):
        super().__init__(dim)
        self.column_writes = []

    def set_column(self, column, slots, tags, cells):
        self.column_writes.append((column, None if slots is None else np.array(slots), np.array(tags), np.array(cells)))


def decoded(col_set, key, n):
    col = col_set.get(key)
    assert col.tags.shape == (n,) and col.cells.shape == (n,), (key, col.tags.shape, n)
    return [col.value_at(s) for s in range(n)]


def test_mirrors_maintained_through_a_write_sequence_equal_columns_built_from_scratch():
    from codd_query_engine_amd import KnnClient

    keys = ["color", "size", "weight", "flag", "mixed", "namespace"]
    client = KnnClient(engine_factory=lambda dim: ColumnEngine(dim), device_where=True)
    col, vecs, mds = cases.random_collection(400, seed=3, client=client)
    for key in keys:   # what the first device-routed filter that names the key does
        built = col._columns.build(key, col._metadatas)
        col._engine.set_column(built.index, None, built.tags, built.cells)
    rng = np.random.default_rng(4)
    vec = lambda n: rng.standard_normal((n, cases.DIM)).astype(np.float32)  # noqa: E731
    # new ids with metadata, new ids without, replaced metadata (some dicts lose keys, one becomes None), metadatas=None on old ids
    col.upsert(ids=[f"new{i}" for i in range(30)], embeddings=vec(30), metadatas=[cases.random_metadata(rng, i) for i in range(30)])
    col.upsert(ids=[f"bare{i}" for i in range(5)], embeddings=vec(5))
    col.upsert(ids=["id3", "id4", "id5", "id6"], embeddings=vec(4), metadatas=[{"color": "teal"}, {"size": 2.5, "flag": False}, None, {}])
    before = [dict(col._metadatas[col._slot_of[i]] or {}) for i in ("id7", "id8")]
    col.upsert(ids=["id7", "id8"], embeddings=vec(2))
    assert [dict(col._metadatas[col._slot_of[i]] or {}) for i in ("id7", "id8")] == before
    col.delete(ids=[f"id{i}" for i in range(100, 180)] + ["new3", "bare1"])
    col.upsert(ids=["id100", "late"], embeddings=vec(2), metadatas=[{"color": "red", "mixed": True}, {"mixed": 1}])   # a deleted id comes back in a fresh slot
    n = len(col._ids)
    live = [s for s in range(n) if col._ids[s] is not None]
    fresh = cases.build_columns(col, keys)
    for key in keys:   # (a tombstone keeps its last cell in the mirror and is absent in a rebuild: the live slots must agree)
        got, want = decoded(col._columns, key, n), decoded(fresh, key, n)
        assert [got[s] for s in live] == [want[s] for s in live], key
    # the engine was told exactly what the mirrors hold: its column after every write so far, replayed (new slots read absent)
    for key in keys:
        mirror = col._columns.get(key)
        tags, cells = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        for column, slots, t, c in col._engine.column_writes:
            if column == mirror.index:
                at = np.arange(t.shape[0]) if slots is None else slots
                tags[at], cells[at] = t, c
        assert np.array_equal(tags, mirror.tags) and np.array_equal(cells, mirror.cells), key
    col.compact()
    n = len(col._ids)
    assert n == col.count() and None not in col._ids
    fresh = cases.build_columns(col, keys)
    for key in keys:
        assert decoded(col._columns, key, n) == decoded(fresh, key, n), key
    # ... and a value without a cell retires its column, on both sides, without disturbing the others
    col.upsert(ids=["nan"], embeddings=vec(1), metadatas=[{"size": float("nan"), "color": "red"}])
    assert col._columns.get("size").host_only and not col._columns.get("color").host_only
    assert col._columns.get("color").value_at(col._slot_of["nan"]) == (wc.TAG_STR, "red")


def test_appending_grows_the_mirrors_by_half_not_by_one_upsert():
    cs = wc.ColumnSet()
    col = cs.build("k", [{"k": i} for i in range(5000)])
    stores, want = set(), [wc.number_key(i) for i in range(5000)]
    for step in range(400):   # 400 appends of 10 slots: a copy per append would be 400 stores
        n = 5000 + 10 * (step + 1)
        cs.resize(n)
        assert col.tags.shape == col.cells.shape == (n,) and not col.tags[n - 10:].any() and not col.cells[n - 10:].any()
        cs.wrote(col, np.arange(n - 10, n), np.full(10, wc.TAG_NUMBER, dtype=np.uint8), np.full(10, 7, dtype=np.uint64))
        stores.add(id(col._tag_store))
    assert len(stores) <= 3 and col.cells[:5000].tolist() == want and (col.cells[5000:] == 7).all()
    cs.resize(6000)   # slots given up and taken again read absent
    cs.resize(9000)
    assert not col.tags[6000:].any() and not col.cells[6000:].any() and (col.cells[5000:6000] == 7).all()
    cs.compacted(np.arange(0, 9000, 2))
    assert col.tags.shape == (4500,) and col.cells[:2500].tolist() == want[::2]


def test_the_module_imports_neither_torch_nor_the_native_library():
    import ast

    tree = ast.parse(open(wc.__file__, encoding="utf-8").read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, "where_columns imports nothing of the package"
            names.add(node.module.split(".")[0])
    assert names <= {"__future__", "numpy", "struct", "typing"}, names
    assert names <= set(sys.stdlib_module_names) | {"numpy"}
