"""Shared by the tests of `where=` on the device: a seeded collection whose metadata has everything the column
encoding must tell apart, a set of filters over it, a numpy interpreter of a compiled program (the kernel's meaning, restated
without the kernel), and the packing of a bool mask into the words the engine returns.  The REFERENCE of every comparison is
Collection._eval_where, the host route that exists without any of this."""

from __future__ import annotations

import numpy as np

from codd_query_engine_amd import KnnClient
from codd_query_engine_amd import where_columns as wc
from tests._masked_oracle_engine import MaskedOracleEngine

DIM = 8
COLORS = ["red", "green", "blue", "amber", "Zebra", "", "grün"]


def host_client(**kw):
    """A façade on the checker engine: search_masked, no eval_where — every filter takes the host route."""
    return KnnClient(engine_factory=lambda dim: MaskedOracleEngine(dim), **kw)


def random_metadata(rng, i: int):
    """Missing keys, keys of mixed classes, bools beside ints, duplicates, +-0.0, +-inf, denormals and the edges of float64's ints."""
    if rng.random() < 0.08:
        return None
    md = {}
    if rng.random() < 0.9:
        md["color"] = COLORS[int(rng.integers(len(COLORS)))]
    if rng.random() < 0.85:
        md["size"] = int(rng.integers(-5, 6))                         # few distinct ints: many duplicates
    if rng.random() < 0.8:
        md["weight"] = [float(rng.standard_normal()), -0.0, 0.0, float("inf"), float("-inf"), 5e-324, -5e-324, float(2**53), float(-2**53),
                        0.5][int(rng.integers(10))] if rng.random() < 0.3 else float(np.round(rng.standard_normal(), 1))
    if rng.random() < 0.7:
        md["flag"] = bool(rng.integers(2))
    if rng.random() < 0.8:                                            # one key, every class: True beside 1, 1.0 beside 1, "1" beside both
        md["mixed"] = [True, False, 1, 0, 1.0, 2, "1", "x", -0.0, 2**53, -(2**53)][int(rng.integers(11))]
    if i % 3 == 0:
        md["namespace"] = f"ns{i % 4}"
    return md


def document_of(md, i: int):
    """A short document that says what the metadata says (every ninth record has none)."""
    return None if i % 9 == 4 else " ".join(f"{k}={v}" for k, v in sorted((md or {}).items())) + f" #{i}"


def random_collection(n: int, seed: int, client=None, name="c", metadata=None, deleted=0, documents=False):
    """(collection, vectors, metadatas) of n records id0 .. id<n-1>; `deleted` of them are deleted afterwards (no auto-compaction
    as long as that is under half)."""
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    mds = [random_metadata(rng, i) for i in range(n)]
    col = (client or host_client()).get_or_create_collection(name, metadata=metadata)
    col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=mds,
               documents=[document_of(md, i) for i, md in enumerate(mds)] if documents else None)
    if deleted:
        col.delete(ids=[f"id{int(i)}" for i in rng.choice(n, size=deleted, replace=False)])
    return col, vecs, mds


# every operator on every class, negated leaves on absent keys, constant-false leaves, mixed-class lists, nesting three deep
FILTERS = [
    {"color": "red"},
    {"color": {"$eq": ""}},
    {"color": {"$ne": "green"}},
    {"color": {"$in": ["red", "blue", "nobody has this"]}},
    {"color": {"$nin": ["red", "grün"]}},
    {"color": {"$eq": "nobody has this"}},                              # an unknown str: a leaf without literals, constant false
    {"color": {"$ne": "nobody has this"}},                              # ... negated: every live record
    {"color": {"$gt": "blue"}},
    {"color": {"$gte": "blue"}},
    {"color": {"$lt": "green"}},
    {"color": {"$lte": "Zebra"}},
    {"size": 3},
    {"size": {"$eq": 3.0}},
    {"size": {"$ne": 0}},
    {"size": {"$gt": 2}},
    {"size": {"$gte": 2}},
    {"size": {"$lt": -1.5}},
    {"size": {"$lte": -5}},
    {"size": {"$in": [1, 2.0, 17]}},
    {"size": {"$nin": [-5, 5]}},
    {"weight": {"$gt": 0.0}},                                           # -0.0 and +0.0 agree: neither is above 0
    {"weight": {"$gte": -0.0}},
    {"weight": {"$eq": 0}},
    {"weight": {"$lt": float("inf")}},
    {"weight": {"$lte": float("-inf")}},
    {"weight": {"$gt": 2**53 - 1}},
    {"weight": {"$lt": 5e-324}},
    {"weight": {"$in": [float("inf"), -(2**53), 0.5]}},
    {"flag": True},
    {"flag": {"$ne": True}},
    {"flag": {"$gt": False}},
    {"flag": {"$gte": False}},
    {"flag": {"$lt": False}},                                           # nothing is below False: constant false
    {"flag": {"$lte": False}},
    {"flag": {"$in": [True, False]}},
    {"flag": {"$nin": [False]}},
    {"mixed": True},
    {"mixed": 1},
    {"mixed": "1"},
    {"mixed": {"$ne": 1}},
    {"mixed": {"$in": [True, 0, "x"]}},                                 # one leaf per class
    {"mixed": {"$nin": [False, 1.0, "1", "unknown"]}},
    {"mixed": {"$gt": 0}},
    {"mixed": {"$gte": "1"}},
    {"mixed": {"$lt": True}},
    {"mixed": {"$eq": 2**53}},
    {"nobody": {"$eq": 1}},                                             # a key no record carries
    {"nobody": {"$ne": 1}},
    {"nobody": {"$nin": ["a", 2]}},
    {"namespace": {"$ne": "ns0"}},
    {"$and": [{"size": {"$gt": -2}}, {"size": {"$lt": 3}}]},            # two leaves, one column
    {"$or": [{"color": "red"}, {"flag": True}, {"nobody": {"$ne": 0}}]},
    {"$and": [{"$or": [{"color": {"$in": ["red", "amber"]}}, {"$and": [{"size": {"$gte": 0}}, {"flag": {"$ne": True}}]}]},
              {"$or": [{"weight": {"$lt": 0}}, {"mixed": {"$nin": [1, "x"]}}, {"$and": [{"flag": True}, {"color": {"$gt": "a"}}]}]},
              {"size": {"$ne": 4}}]},
    {"$or": [{"$and": [{"color": "red"}, {"color": "blue"}]}, {"size": {"$in": [99]}}]},   # nobody
]

# filters that cannot run on the device: the compiler returns None and the façade takes the host route
HOST_FILTERS = [
    {"size": {"$eq": float("nan")}},
    {"size": {"$gt": 2**53 + 1}},
    {"size": {"$in": [1, 10**400]}},
    {"$and": [{"color": "red"}, {"weight": {"$lt": float("nan")}}]},
]


def pack(mask: np.ndarray) -> np.ndarray:
    """bool over the row slots -> ceil(n / 32) uint32 words, bit r & 31 of word r >> 5 = row slot r."""
    n = mask.shape[0]
    words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
    packed = np.packbits(mask, bitorder="little")
    words[: packed.shape[0]] = packed
    return words.view("<u4")


def interpret(program, columns, live: np.ndarray) -> np.ndarray:
    """A compiled program over the numpy mirrors: what where_eval_kernel computes, restated.  columns: engine column number ->
    where_columns.Column; live: bool over the row slots."""
    leaf_pass = []
    lits = np.asarray(program.literals, dtype=np.uint64)
    for column, tag, kind, negate, first, count in program.leaves:
        col = columns[column]
        cells = col.cells
        mine = lits[first : first + count]
        if kind == wc.KIND_IN:
            hit = np.isin(cells, mine)
        else:
            hit = {wc.KIND_LT: cells < mine[0], wc.KIND_LE: cells <= mine[0], wc.KIND_GT: cells > mine[0], wc.KIND_GE: cells >= mine[0]}[kind]
        ok = (col.tags == tag) & hit
        leaf_pass.append(~ok if negate else ok)
    stack = []
    for op in program.ops:
        if op == wc.OP_AND or op == wc.OP_OR:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b if op == wc.OP_AND else a | b)
        else:
            stack.append(leaf_pass[op])
    assert len(stack) == 1
    return stack[0] & live


def build_columns(col, keys) -> wc.ColumnSet:
    """Columns built from scratch over a collection's records, for the given keys."""
    cs = wc.ColumnSet()
    for key in keys:
        cs.build(key, col._metadatas)
    return cs
