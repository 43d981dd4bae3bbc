"""
KnnClient / Collection — the chromadb-shaped object the store is constructed with.

The reference injects a `chromadb` client into MetricsSemanticMetadataStore
(store.py:43-57) and calls exactly: client.get_or_create_collection (store.py:60-69),
client.heartbeat (codd_jobs/metrics_semantic_indexer_main.py:215,330), collection.upsert
(store.py:236-238), collection.get (store.py:260), collection.query (store.py:314-316).
This module answers those calls with Chroma-shaped dicts, keeps ids / documents / metadata
on the host (string bookkeeping, not arithmetic) and sends every vector operation through
the C ABI of the HIP engine (knn_index.DeviceKnnIndex).  There is no CPU search path: the
default engine factory raises if the library or the GPU is missing.

`engine_factory(dim) -> engine` exists so that host-logic tests can stand the façade on a
checker engine of their own (tests/_oracle_engine.py); products never pass it.  A factory that can
build engines for ChromaDB's other spaces says so with a `spaces` attribute (names of
native.METRIC_CODES) and is then called as `engine_factory(dim, space=...)` for a collection whose
metadata asks for one of them; a factory without the attribute serves cosine only.

Spaces (`metadata={"hnsw:space": ...}`): "cosine" (the default here), "l2" (squared
distance) and "ip" (1 - inner product), ChromaDB's definitions.  A non-cosine collection stores the
embeddings as given (upsert with normalize=False) and `query` returns that space's distances;
everything else — namespaces, `where`, `where_document`, delete, compact, persistence — is the same.
`metadata={"hnsw:space": "l2", "codd:space_filter": 1}` switches on the engine's int8 filter leg for
such a collection (large batches, same answers), when the engine is created and again
after `reload`; an engine without `set_option` ignores it.  `"codd:space_ivf": 1` sets the engine's
"space_ivf" option the same way (codd_query_engine_amd.ivf accepts that engine; `query`
itself never takes the IVF route).

Persistence (`KnnClient(path=...)`, the role of `SemanticStoreConfig.chromadb_path`, declared and
never read in the reference, codd_lib/codd_lib/config/semantic_store_config.py:13): the indexer job
and the service are different processes that share state only through the Chroma server; here they
share a directory.  Layout per collection:

    <path>/<collection>/CURRENT            name of the live generation (replaced atomically, last)
    <path>/<collection>/gen-<n>/manifest.json   name, metadata, dim, padded_dim, dtype, count
                               /rows.bin        stored rows exactly as they sit in HBM
                               /ids.json, metadatas.jsonl, documents.jsonl

`persist()` writes a new generation and flips CURRENT; `reload()` picks up a newer generation.
Deleted records never reach the disk: `persist()` compacts a collection before it writes it.
"""

from __future__ import annotations

import json
import os
import re
import shutil
import time
from typing import Any, Callable, Optional, Sequence

import numpy as np

from . import regex_dfa, where_columns
from .embedding import EmbeddingFunction, HashingEmbeddingFunction

_DEFAULT_SPACE = "cosine"
_ALL_SPACES = ("cosine", "l2", "ip")
FORMAT_VERSION = 1  # of the on-disk layout


def _default_engine_factory(device: str, dtype: str) -> Callable[..., Any]:
    def make(dim: int, space: str = _DEFAULT_SPACE):
        from .knn_index import DeviceKnnIndex  # raises NativeLibraryError without .so / GPU

        return DeviceKnnIndex(dim, dtype=dtype, device=device, space=space)

    make.spaces = _ALL_SPACES
    return make


def _factory_spaces(engine_factory) -> tuple:
    """The spaces a factory builds engines for: its `spaces` attribute, cosine only without one."""
    return tuple(getattr(engine_factory, "spaces", (_DEFAULT_SPACE,)))


_SPACE_FILTER_KEY = "codd:space_filter"
_SPACE_IVF_KEY = "codd:space_ivf"
_DOCUMENT_REGEX_KEY = "codd:document_regex"   # collection metadata: 1 = where_document knows $regex / $not_regex
_DEVICE_WHERE_KEY = "codd:device_where"       # collection metadata: 1 = general `where` filters are evaluated on the engine's device


def _space_of(metadata: Optional[dict]) -> str:
    return (metadata or {}).get("hnsw:space", _DEFAULT_SPACE)


class Collection:
    """One named set of (id, document, metadata, embedding) rows.

    Row slots are assigned in first-insertion order, so "ties -> lower row" means "ties -> the id
    inserted first".  A deleted record's slot becomes a tombstone (its id is None in the host lists, the
    engine never returns it) and is not reused: an id that is deleted and upserted again takes a fresh
    slot at the end, a new insertion for the tie rule.  compact() squeezes the tombstones out; the live
    rows keep their relative order, so the tie rule survives it.
    """

    AUTO_COMPACT_SHARE = 0.5  # compact() runs by itself once dead slots exceed this share of all slots
    # Texts per call from which query_texts / documents are embedded on the engine's device (embed_on_device) instead of on the host.
    # Measured (profiles/embed/README.md): one text costs the same on both routes, from two on the device route wins.
    DEVICE_EMBED_MIN_TEXTS = 2

    def __init__(self, name: str, metadata: Optional[dict], embedding_function: EmbeddingFunction,
                 engine_factory: Callable[[int], Any], document_regex: bool = False, device_where: bool = False):
        self.name = name
        self._client_document_regex = bool(document_regex)   # KnnClient(document_regex=True): the opt-in without the metadata key
        self._client_device_where = bool(device_where)       # KnnClient(device_where=True): likewise
        self.metadata = dict(metadata or {})
        self._embed = embedding_function
        self._engine_factory = engine_factory
        self._engine = None
        self._ids: list[Optional[str]] = []  # by row slot; None = deleted (tombstone until compact())
        self._slot_of: dict[str, int] = {}
        self._documents: list[Optional[str]] = []
        self._metadatas: list[Optional[dict]] = []
        self._dirty = False
        self._generation = 0
        self._scope_of_namespace: dict[str, int] = {}  # namespace string -> scope label of the engine (from 1, first seen first)
        # general `where`: per metadata key, (value class, value) -> row slots, built on first use; compiled masks by canonical filter.
        # Both are dropped by every upsert / delete / compact / load.
        self._key_index: dict[str, dict[tuple, np.ndarray]] = {}
        self._mask_cache: dict[str, np.ndarray] = {}
        # `where_document`: host masks by canonical filter; on a device engine the needles' bitmaps (packed words on the GPU) by needle
        # bytes, and whether the engine holds the current documents.  Dropped with the two above.
        self._doc_mask_cache: dict[str, np.ndarray] = {}
        # ... and under ("re", pattern) a $regex pattern's, under ("has document",) the records that have one
        self._doc_bits_cache: dict[Any, Any] = {}
        self._docs_on_device = False
        self._docs_fit_device: Optional[bool] = None   # no document holds NUL (None: not looked yet; one pass per change)
        self._docs_ascii: Optional[bool] = None        # every document is ASCII (found by the same pass)
        # `where` on the device (opt-in): the metadata columns built so far — numpy mirrors of the engine's, kept in step
        # by every write, dropped by a load — and the filters' bitmaps (packed words on the GPU) by canonical filter, dropped by writes
        self._columns = where_columns.ColumnSet()
        self._where_bits_cache: dict[str, Any] = {}

    # ------------------------------------------------------------------ helpers
    @property
    def space(self) -> str:
        """The collection's `hnsw:space`: "cosine" unless its metadata names another."""
        return _space_of(self.metadata)

    def _make_engine(self, dim: int, space: str, metadata: Optional[dict] = None):
        """A new engine of `space` from the factory; a cosine one by the plain call every factory answers.  `metadata`: the
        collection metadata whose engine options apply (default: this collection's)."""
        if space == _DEFAULT_SPACE:
            engine = self._engine_factory(dim)
        else:
            if space not in _factory_spaces(self._engine_factory):
                raise ValueError(f"hnsw:space={space!r} is not on this path (supported: {_factory_spaces(self._engine_factory)})")
            engine = self._engine_factory(dim, space=space)
            if getattr(engine, "space", space) != space:
                raise ValueError(f"the engine factory answered space {engine.space!r} for {space!r}")
        self._apply_engine_options(engine, self.metadata if metadata is None else metadata)
        return engine

    @staticmethod
    def _apply_engine_options(engine, metadata: Optional[dict]) -> None:
        """Collection metadata that is an engine option: "codd:space_filter" (the int8 filter leg of an ip or l2
        collection) -> engine.set_option("space_filter", value); "codd:space_ivf" (IVF on such an engine) ->
        engine.set_option("space_ivf", value).  Skipped on an engine without set_option."""
        for key, option in ((_SPACE_FILTER_KEY, "space_filter"), (_SPACE_IVF_KEY, "space_ivf")):
            value = (metadata or {}).get(key)
            if value is not None and callable(getattr(engine, "set_option", None)):
                engine.set_option(option, int(value))

    def _engine_for(self, dim: int):
        if self._engine is None:
            self._engine = self._make_engine(dim, self.space)
        elif self._engine.dim != dim:
            raise ValueError(f"embedding dimension {dim} does not match collection dimension {self._engine.dim}")
        return self._engine

    @staticmethod
    def _as_matrix(embeddings) -> np.ndarray:
        m = np.asarray(embeddings, dtype=np.float32)
        if m.ndim == 1:
            m = m[None, :]
        if m.ndim != 2:
            raise ValueError("embeddings must be [n, d]")
        return np.ascontiguousarray(m)

    def count(self) -> int:
        """Live records (deleted ones do not count)."""
        return len(self._slot_of)

    # ------------------------------------------------------------------ text -> vector on the engine's device
    def _embeds_on_device(self, engine, engine_method: str, n_texts: int) -> bool:
        """The routing rule of DESIGN.md §19: the embedder can embed on a device, the engine lives on one and takes device tensors
        through `engine_method`, and the batch is large enough for the device route to be the faster one."""
        return (hasattr(self._embed, "embed_on_device") and engine is not None and hasattr(engine, engine_method)
                and getattr(engine, "device", None) is not None and n_texts >= self.DEVICE_EMBED_MIN_TEXTS)

    @staticmethod
    def _rows_of(q, members):
        """q[members] for the host matrix or the device tensor the queries are (members: row numbers or a bool mask)."""
        if isinstance(q, np.ndarray):
            return q[members]
        import torch

        return q[torch.as_tensor(np.asarray(members), device=q.device)]

    # ------------------------------------------------------------------ namespaces -> scopes
    def _scope_for(self, metadata: Optional[dict]) -> int:
        """The engine's scope label of a row with this metadata: 0 without a "namespace" key."""
        if not metadata or "namespace" not in metadata:
            return 0
        ns = metadata["namespace"]
        scope = self._scope_of_namespace.get(ns)
        if scope is None:
            scope = len(self._scope_of_namespace) + 1
            self._scope_of_namespace[ns] = scope
        return scope

    _WHERE_FORMS = 'where={"namespace": "x"}, where={"namespace": {"$eq": "x"}}, or a list of one such dict / None per query'

    @classmethod
    def _where_namespace(cls, where) -> Optional[str]:
        if where is None:
            return None
        if isinstance(where, dict) and list(where) == ["namespace"]:
            cond = where["namespace"]
            if isinstance(cond, str):
                return cond
            if isinstance(cond, dict) and list(cond) == ["$eq"] and isinstance(cond["$eq"], str):
                return cond["$eq"]
        raise ValueError(f"unsupported where filter {where!r}; supported: {cls._WHERE_FORMS}")

    # ------------------------------------------------------------------ general where -> row mask
    _COMPARISONS = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte")
    _MASK_CACHE_SIZE = 32
    _WHERE_GRAMMAR = ('{"key": value}, {"key": {"$eq"|"$ne"|"$gt"|"$gte"|"$lt"|"$lte": value}}, {"key": {"$in"|"$nin": [values]}}, '
                      '{"$and"|"$or": [filters]}; values are str / int / float / bool')

    def _where_error(self, where, why: str) -> ValueError:
        return ValueError(f"unsupported where filter {where!r}: {why}; supported: {self._WHERE_FORMS}, and on an engine with masked search "
                          f"{self._WHERE_GRAMMAR}")

    @staticmethod
    def _value_class(v) -> Optional[str]:
        """'b' bool, 'n' int / float, 's' str; None for anything else.  Values only ever meet values of their own class."""
        if isinstance(v, bool):
            return "b"
        if isinstance(v, (int, float)):
            return "n"
        return "s" if isinstance(v, str) else None

    def _check_where(self, where, top=None) -> None:
        """ValueError unless `where` is a filter of ChromaDB's metadata grammar."""
        top = where if top is None else top
        if not isinstance(where, dict) or len(where) != 1:
            raise self._where_error(top, "a filter is a dict with exactly one key")
        (key, cond), = where.items()
        if not isinstance(key, str):
            raise self._where_error(top, "keys are strings")
        if key in ("$and", "$or"):
            if not isinstance(cond, (list, tuple)) or len(cond) == 0:
                raise self._where_error(top, f"{key} takes a non-empty list of filters")
            for sub in cond:
                self._check_where(sub, top)
            return
        if key.startswith("$"):
            raise self._where_error(top, f"unknown operator {key}")
        if not isinstance(cond, dict):
            cond = {"$eq": cond}
        if len(cond) != 1:
            raise self._where_error(top, "a condition is a value or a dict with exactly one operator")
        (op, val), = cond.items()
        if op in ("$in", "$nin"):
            if not isinstance(val, (list, tuple)) or len(val) == 0 or any(self._value_class(v) is None for v in val):
                raise self._where_error(top, f"{op} takes a non-empty list of str / int / float / bool")
        elif op in self._COMPARISONS:
            if self._value_class(val) is None:
                raise self._where_error(top, f"{op} takes a str / int / float / bool")
        else:
            raise self._where_error(top, f"unknown operator {op!r}")

    def _index_of_key(self, key: str) -> dict[tuple, np.ndarray]:
        """(value class, value) -> ascending row slots of the live records that carry `key` with that value."""
        index = self._key_index.get(key)
        if index is None:
            found: dict[tuple, list[int]] = {}
            for slot, md in enumerate(self._metadatas):
                if md and key in md and self._ids[slot] is not None:
                    cls = self._value_class(md[key])
                    if cls is not None:
                        found.setdefault((cls, md[key]), []).append(slot)
            index = {kv: np.asarray(slots, dtype=np.int64) for kv, slots in found.items()}
            self._key_index[key] = index
        return index

    def _eval_where(self, where) -> np.ndarray:
        (key, cond), = where.items()
        n = len(self._ids)
        if key in ("$and", "$or"):
            masks = [self._eval_where(sub) for sub in cond]
            return np.logical_and.reduce(masks) if key == "$and" else np.logical_or.reduce(masks)
        (op, val), = (cond if isinstance(cond, dict) else {"$eq": cond}).items()
        index = self._index_of_key(key)
        mask = np.zeros(n, dtype=bool)
        if op in ("$eq", "$ne", "$in", "$nin"):
            for v in (val if op in ("$in", "$nin") else [val]):
                slots = index.get((self._value_class(v), v))
                if slots is not None:
                    mask[slots] = True
            if op in ("$ne", "$nin"):  # (a record without the key passes; a deleted slot never does)
                live = np.fromiter((doc_id is not None for doc_id in self._ids), dtype=bool, count=n)
                mask = live & ~mask
            return mask
        cls = self._value_class(val)
        test = {"$gt": lambda a: a > val, "$gte": lambda a: a >= val, "$lt": lambda a: a < val, "$lte": lambda a: a <= val}[op]
        for (c, stored), slots in index.items():  # (the key's distinct values, not its records)
            if c == cls and test(stored):
                mask[slots] = True
        return mask

    def _where_mask(self, where) -> np.ndarray:
        """The checked filter as a bool array over the row slots (deleted slots False); cached by the filter's canonical JSON."""
        canon = json.dumps(where, sort_keys=True, ensure_ascii=False)
        mask = self._mask_cache.get(canon)
        if mask is None:
            mask = self._eval_where(where)
            if len(self._mask_cache) >= self._MASK_CACHE_SIZE:
                self._mask_cache.pop(next(iter(self._mask_cache)))
            self._mask_cache[canon] = mask
        return mask

    def _forget_where_index(self) -> None:
        self._where_bits_cache.clear()   # (the columns themselves survive writes: upsert and compact maintain them)
        self._key_index.clear()
        self._mask_cache.clear()
        self._doc_mask_cache.clear()
        self._doc_bits_cache.clear()
        self._docs_on_device = False
        self._docs_fit_device = None
        self._docs_ascii = None

    # ------------------------------------------------------------------ general where -> row bitmap on the device (opt-in)
    @property
    def device_where(self) -> bool:
        """Whether a general `where` is evaluated on the engine's device here: the collection's metadata says so
        ("codd:device_where": 1), or its client does."""
        return self._client_device_where or bool(self.metadata.get(_DEVICE_WHERE_KEY))

    def _has_device_where(self) -> bool:
        return self.device_where and all(hasattr(self._engine, m) for m in ("eval_where", "set_column", "search_masked_dev"))

    def _drop_columns(self) -> None:
        if len(self._columns) and self._engine is not None and hasattr(self._engine, "drop_columns"):
            self._engine.drop_columns()
        self._columns.clear()

    def _where_bits(self, where):
        """The checked filter as packed words on the engine's device — the live row slots that satisfy it, match_documents' form —
        from the 32-entry cache or evaluated now by the engine's predicate kernel over the metadata columns; a key's column is built
        by the first filter that names it (one pass over the records, one upload).  None: this filter runs on the host (a
        host_only column, a literal without a key, a program beyond the limits; where_columns.compile_where)."""
        canon = json.dumps(where, sort_keys=True, ensure_ascii=False)
        bits = self._where_bits_cache.get(canon)
        if bits is not None:
            return bits
        for key in where_columns.filter_keys(where):
            col = self._columns.get(key)
            if col is None:
                col = self._columns.build(key, self._metadatas)
                if not col.host_only:
                    try:
                        self._engine.set_column(col.index, None, col.tags, col.cells)
                    except Exception:
                        self._drop_columns()
                        raise
            if col.host_only:
                return None
        program = where_columns.compile_where(where, self._columns.by_key)
        if program is None:
            return None
        bits = self._engine.eval_where(program)
        if len(self._where_bits_cache) >= self._MASK_CACHE_SIZE:
            self._where_bits_cache.pop(next(iter(self._where_bits_cache)))
        self._where_bits_cache[canon] = bits
        return bits

    def _write_columns(self, slots: np.ndarray, metadatas: Optional[Sequence[Optional[dict]]]) -> None:
        """After an upsert that the engine and the host lists have taken: every column built so far learns the written slots'
        cells — a replaced metadata dict that lacks the key writes "absent"; metadatas=None writes nothing (an existing record
        keeps its metadata, a fresh slot is absent on both sides already).  The engine first, then the mirror."""
        self._columns.resize(len(self._ids))
        if metadatas is None or not len(self._columns):
            return
        try:
            for col, tags, cells in self._columns.encode_slots(metadatas):
                self._engine.set_column(col.index, slots, tags, cells)
                self._columns.wrote(col, slots, tags, cells)
        except Exception:
            self._drop_columns()   # (derived data: the next device-routed filter builds what it needs again)
            raise

    # ------------------------------------------------------------------ where_document -> row mask
    _WHERE_DOCUMENT_GRAMMAR = ('{"$contains": "text"}, {"$not_contains": "text"}, {"$and": [filters]}, {"$or": [filters]}; '
                               'text is a non-empty str, matched case-sensitively as a substring of the stored document')
    # ... on a collection that opted in to regular expressions ("codd:document_regex": 1, or KnnClient(document_regex=True))
    _WHERE_DOCUMENT_GRAMMAR_REGEX = ('{"$contains": "text"}, {"$not_contains": "text"}, {"$regex": "pattern"}, {"$not_regex": "pattern"}, '
                                     '{"$and": [filters]}, {"$or": [filters]}; text is a non-empty str, matched case-sensitively as a substring of '
                                     'the stored document; pattern is a non-empty str that re.compile accepts, matched as re.search(pattern, document)')
    _DEVICE_NEEDLE_MAX = 256  # CODD_KNN_MAX_NEEDLE: longer needles, and needles holding NUL, are evaluated on the host

    @property
    def document_regex(self) -> bool:
        """Whether `where_document` knows $regex / $not_regex here: the collection's metadata says so, or its client does."""
        return self._client_document_regex or bool(self.metadata.get(_DOCUMENT_REGEX_KEY))

    def _where_document_error(self, where_document, why: str) -> ValueError:
        grammar = self._WHERE_DOCUMENT_GRAMMAR_REGEX if self.document_regex else self._WHERE_DOCUMENT_GRAMMAR
        return ValueError(f"unsupported where_document filter {where_document!r}: {why}; supported: {grammar}")

    def _check_where_document(self, wd, top=None) -> None:
        """ValueError unless `wd` is a filter of ChromaDB's document grammar."""
        top = wd if top is None else top
        if not isinstance(wd, dict) or len(wd) != 1:
            raise self._where_document_error(top, "a filter is a dict with exactly one key")
        (op, arg), = wd.items()
        if op in ("$and", "$or"):
            if not isinstance(arg, (list, tuple)) or len(arg) == 0:
                raise self._where_document_error(top, f"{op} takes a non-empty list of filters")
            for sub in arg:
                self._check_where_document(sub, top)
        elif op in ("$contains", "$not_contains"):
            if not isinstance(arg, str) or arg == "":
                raise self._where_document_error(top, f"{op} takes a non-empty str")
        elif op in ("$regex", "$not_regex") and self.document_regex:
            if not isinstance(arg, str) or arg == "":
                raise self._where_document_error(top, f"{op} takes a non-empty str")
            try:
                re.compile(arg)
            except (re.error, RecursionError, OverflowError) as e:
                raise self._where_document_error(top, f"{op} pattern {arg!r} does not compile: {e}") from None
        else:
            raise self._where_document_error(top, f"unknown operator {op!r}")

    @staticmethod
    def _utf8(text: str) -> bytes:
        return text.encode("utf-8", "surrogatepass")

    def _live_mask(self) -> np.ndarray:
        return np.fromiter((doc_id is not None for doc_id in self._ids), dtype=bool, count=len(self._ids))

    def _contains_mask(self, needle: str) -> np.ndarray:
        """bool over the row slots: the stored document contains `needle` (a record without a document contains nothing)."""
        return np.fromiter((doc is not None and needle in doc for doc in self._documents), dtype=bool, count=len(self._documents))

    def _regex_mask(self, pattern: str) -> np.ndarray:
        """bool over the row slots: re.search(pattern, document) finds something (a record without a document matches nothing)."""
        search = re.compile(pattern).search
        return np.fromiter((doc is not None and search(doc) is not None for doc in self._documents), dtype=bool, count=len(self._documents))

    def _eval_where_document(self, wd) -> np.ndarray:
        (op, arg), = wd.items()
        if op in ("$and", "$or"):
            masks = [self._eval_where_document(sub) for sub in arg]
            return np.logical_and.reduce(masks) if op == "$and" else np.logical_or.reduce(masks)
        hit = self._regex_mask(arg) if op in ("$regex", "$not_regex") else self._contains_mask(arg)
        return hit if op in ("$contains", "$regex") else self._live_mask() & ~hit   # (a deleted slot never passes)

    def _where_document_mask(self, wd) -> np.ndarray:
        """The checked filter as a bool array over the row slots, evaluated on the host (`needle in doc`); cached by canonical JSON."""
        canon = json.dumps(wd, sort_keys=True, ensure_ascii=True)
        mask = self._doc_mask_cache.get(canon)
        if mask is None:
            mask = self._eval_where_document(wd)
            if len(self._doc_mask_cache) >= self._MASK_CACHE_SIZE:
                self._doc_mask_cache.pop(next(iter(self._doc_mask_cache)))
            self._doc_mask_cache[canon] = mask
        return mask

    # the device path: needles matched by the engine's kernel, bitmaps combined where they are
    def _has_device_documents(self) -> bool:
        return hasattr(self._engine, "match_documents") and hasattr(self._engine, "search_masked_dev")

    def _words_on_device(self, mask: np.ndarray):
        """A bool mask over the row slots as packed words on the engine's device (int32 tensor, match_documents' form)."""
        import torch

        n = mask.shape[0]
        words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
        packed = np.packbits(mask, bitorder="little")
        words[: packed.shape[0]] = packed
        return torch.from_numpy(words.view("<i4")).to(self._engine.device)

    def _needle_bits(self, needle: str):
        """The bitmap of one $contains needle on the device, from the 32-entry cache or matched now (the first use after a change
        uploads the document snapshot)."""
        raw = self._utf8(needle)
        bits = self._doc_bits_cache.get(raw)
        if bits is None:
            if len(raw) > self._DEVICE_NEEDLE_MAX or b"\x00" in raw:
                bits = self._words_on_device(self._contains_mask(needle))
            else:
                if not self._docs_on_device:
                    self._engine.set_documents([None if doc is None else self._utf8(doc) for doc in self._documents])
                    self._docs_on_device = True
                bits = self._engine.match_documents(raw)
            if len(self._doc_bits_cache) >= self._MASK_CACHE_SIZE:
                self._doc_bits_cache.pop(next(iter(self._doc_bits_cache)))
            self._doc_bits_cache[raw] = bits
        return bits

    def _cache_doc_bits(self, key, bits):
        if len(self._doc_bits_cache) >= self._MASK_CACHE_SIZE:
            self._doc_bits_cache.pop(next(iter(self._doc_bits_cache)))
        self._doc_bits_cache[key] = bits
        return bits

    def _has_document_bits(self):
        """The records that have a document, as words on the device (the arena stores None as an empty document)."""
        bits = self._doc_bits_cache.get(("has document",))
        if bits is None:
            has = np.fromiter((doc is not None for doc in self._documents), dtype=bool, count=len(self._documents))
            bits = self._cache_doc_bits(("has document",), self._words_on_device(has))
        return bits

    def _regex_bits(self, pattern: str):
        """The bitmap of one $regex pattern on the device, from the cache (under ("re", pattern): no needle's bytes) or made now.
        A pattern that is plain text after parsing is a needle (doc_match_kernel); one inside the device subset runs as a byte
        DFA (regex_dfa.compile_search_dfa, doc_regex_kernel); any other is evaluated here by re and uploaded as a mask."""
        key = ("re", pattern)
        bits = self._doc_bits_cache.get(key)
        if bits is not None:
            return bits
        text = regex_dfa.literal_of(pattern)
        if text is not None:
            return self._cache_doc_bits(key, self._needle_bits(text))
        dfa = regex_dfa.compile_search_dfa(pattern, bool(self._docs_ascii)) if hasattr(self._engine, "match_documents_dfa") else None
        if dfa is None:
            return self._cache_doc_bits(key, self._words_on_device(self._regex_mask(pattern)))
        if not self._docs_on_device:
            self._engine.set_documents([None if doc is None else self._utf8(doc) for doc in self._documents])
            self._docs_on_device = True
        bits = self._engine.match_documents_dfa(dfa)
        # the arena holds a record without a document as an empty one: where the pattern matches "", such records are taken out
        if re.search(pattern, "") is not None and any(doc is None and doc_id is not None for doc, doc_id in zip(self._documents, self._ids)):
            bits = bits & self._has_document_bits()
        return self._cache_doc_bits(key, bits)

    def _where_document_bits(self, wd):
        (op, arg), = wd.items()
        if op in ("$and", "$or"):
            parts = [self._where_document_bits(sub) for sub in arg]
            out = parts[0]
            for part in parts[1:]:
                out = out & part if op == "$and" else out | part
            return out
        bits = self._regex_bits(arg) if op in ("$regex", "$not_regex") else self._needle_bits(arg)
        return bits if op in ("$contains", "$regex") else ~bits   # (the engine clips the words to the count and drops dead rows)

    def _documents_fit_device(self) -> bool:
        """The engine's arena separates documents by NUL: a collection whose documents hold one is filtered on the host.  One pass
        over the documents per change of the collection (the flag is dropped with the snapshot's), not one per query.  The same
        pass finds out whether every document is ASCII: the condition for \\d \\w \\s and (?i) in a device pattern."""
        if self._docs_fit_device is None:
            fit = ascii_only = True
            for doc in self._documents:
                if doc is not None:
                    if fit and "\x00" in doc:
                        fit = False
                    if ascii_only and not doc.isascii():
                        ascii_only = False
            self._docs_fit_device, self._docs_ascii = fit, ascii_only
        return self._docs_fit_device

    def _where_scopes(self, where, B: int) -> Optional[np.ndarray]:
        """Per-query scope labels of a `where` (None when no query is restricted); -1 marks a namespace nobody stored."""
        if isinstance(where, (list, tuple)):
            if len(where) != B:
                raise ValueError(f"where has {len(where)} entries for {B} queries; supported: {self._WHERE_FORMS}")
            names = [self._where_namespace(w) for w in where]
        else:
            names = [self._where_namespace(where)] * B
        if all(ns is None for ns in names):
            return None
        return np.array([0 if ns is None else self._scope_of_namespace.get(ns, -1) for ns in names], dtype=np.int64)

    # ------------------------------------------------------------------ writes
    def upsert(self, ids: Sequence[str], embeddings=None, metadatas: Optional[Sequence[Optional[dict]]] = None,
               documents: Optional[Sequence[Optional[str]]] = None) -> None:
        """Insert-or-replace by id (chromadb Collection.upsert; store.py:236-238).  Without `embeddings` the documents are embedded:
        on the engine's device when the embedder has embed_on_device, the engine upsert_device and a device, the call holds at
        least DEVICE_EMBED_MIN_TEXTS documents and every id is new; on the host otherwise.  The same vectors
        either way."""
        ids = list(ids)
        n = len(ids)
        if n == 0:
            return
        if any(not isinstance(i, str) or not i for i in ids):
            raise ValueError("ids must be non-empty strings")
        if len(set(ids)) != n:
            raise ValueError("duplicate ids in one upsert")
        for name, seq in (("metadatas", metadatas), ("documents", documents)):
            if seq is not None and len(seq) != n:
                raise ValueError(f"{name} has {len(seq)} entries for {n} ids")
        if embeddings is None:
            if documents is None or any(d is None for d in documents):
                raise ValueError("upsert needs embeddings or documents to embed")
            # the device route: every id is new, so the rows are the contiguous run of slots from len(self._ids) that upsert_device
            # writes; the width is the embedder's.  Anything else is embedded here and goes through engine.upsert, as before.
            if (hasattr(self._embed, "embed_on_device") and n >= self.DEVICE_EMBED_MIN_TEXTS and not any(i in self._slot_of for i in ids)
                    and self._embeds_on_device(self._engine_for(int(self._embed.dim)), "upsert_device", n)):
                vecs = self._embed.embed_on_device(list(documents), self._engine.device)
            else:
                vecs = self._as_matrix(self._embed(list(documents)))
        else:
            vecs = self._as_matrix(embeddings)
        if vecs.shape[0] != n:
            raise ValueError(f"{vecs.shape[0]} embeddings for {n} ids")
        engine = self._engine_for(vecs.shape[1])

        slots = np.empty(n, dtype=np.int64)
        next_slot = len(self._ids)
        fresh = []
        for i, doc_id in enumerate(ids):
            slot = self._slot_of.get(doc_id)
            if slot is None:
                slot = next_slot
                next_slot += 1
                fresh.append(doc_id)
            slots[i] = slot
        # device first: host bookkeeping only changes if it succeeded.  (l2 / ip: the vectors are stored as given)
        raw = {} if self.space == _DEFAULT_SPACE else {"normalize": False}
        if isinstance(vecs, np.ndarray):
            engine.upsert(slots, vecs, **raw)
        else:
            engine.upsert_device(int(slots[0]), vecs, **raw)
        for doc_id in fresh:
            self._slot_of[doc_id] = len(self._ids)
            self._ids.append(doc_id)
            self._documents.append(None)
            self._metadatas.append(None)
        for i, slot in enumerate(slots.tolist()):
            if documents is not None:
                self._documents[slot] = documents[i]
            if metadatas is not None:
                self._metadatas[slot] = dict(metadatas[i]) if metadatas[i] is not None else None
        self._dirty = True
        self._forget_where_index()
        # the rows' namespaces as scope labels of the engine (an engine without scoped search is not asked)
        if metadatas is not None and hasattr(engine, "set_scopes"):
            scopes = np.array([self._scope_for(md) for md in metadatas], dtype=np.uint32)
            if scopes.any() or len(fresh) < n:  # (a new slot starts with scope 0; a rewritten one may have to lose its label)
                engine.set_scopes(slots, scopes)
        self._write_columns(slots, metadatas)   # (nothing to do unless a device-routed `where` has built columns)

    def delete(self, ids: Optional[Sequence[str]] = None, where=None) -> None:
        """chromadb Collection.delete: forget records by id and / or by namespace.

        ids: unknown ids are ignored.  where: the forms `query` accepts for one query ({"namespace": "x"} or
        {"namespace": {"$eq": "x"}}): every record of that namespace.  Both: the intersection.  Neither: ValueError.
        The engine is told first (the rows become tombstones no search returns), then the host lists follow."""
        if ids is None and where is None:
            raise ValueError("delete needs ids and / or where")
        if ids is not None:
            ids = list(ids)
            if any(not isinstance(i, str) or not i for i in ids):
                raise ValueError("ids must be non-empty strings")
        namespace = self._where_namespace(where)
        if self._engine is not None and not hasattr(self._engine, "delete"):
            raise NotImplementedError(f"{type(self._engine).__name__} has no delete: Collection.delete needs an engine with delete / live_count / compact")
        if ids is None:
            slots = [s for s, md in enumerate(self._metadatas) if self._ids[s] is not None and md and md.get("namespace") == namespace]
        else:
            slots = sorted({self._slot_of[i] for i in ids if i in self._slot_of})
            if where is not None:
                slots = [s for s in slots if self._metadatas[s] and self._metadatas[s].get("namespace") == namespace]
        if not slots:
            return
        self._engine.delete(np.asarray(slots, dtype=np.int64))  # device first: host bookkeeping only changes if it succeeded
        for s in slots:
            del self._slot_of[self._ids[s]]
            self._ids[s] = None
            self._documents[s] = None
            self._metadatas[s] = None
        self._dirty = True
        self._forget_where_index()
        if len(self._ids) - len(self._slot_of) > self.AUTO_COMPACT_SHARE * len(self._ids):
            self.compact()

    def compact(self) -> int:
        """Squeeze the tombstones out: the engine moves the live rows to slots 0 .. live-1 in slot order and the host lists are
        renumbered by the same mapping.  Answers do not change.  Returns the number of slots (= live records) afterwards."""
        if len(self._slot_of) == len(self._ids):
            return len(self._ids)
        new_count = self._engine.compact()
        keep = [s for s, doc_id in enumerate(self._ids) if doc_id is not None]
        if new_count != len(keep):
            raise RuntimeError(f"engine compacted to {new_count} rows, the host lists hold {len(keep)} live records")
        self._ids = [self._ids[s] for s in keep]
        self._documents = [self._documents[s] for s in keep]
        self._metadatas = [self._metadatas[s] for s in keep]
        self._slot_of = {doc_id: i for i, doc_id in enumerate(self._ids)}
        self._forget_where_index()
        self._columns.compacted(keep)   # (the engine has moved its copy of the columns with the rows)
        return new_count

    def add(self, ids: Sequence[str], embeddings=None, metadatas=None, documents=None) -> None:
        """chromadb Collection.add: like upsert, but ids already present are left untouched."""
        keep = [i for i, d in enumerate(ids) if d not in self._slot_of]
        if not keep:
            return
        pick = lambda seq: None if seq is None else [seq[i] for i in keep]  # noqa: E731
        emb = None if embeddings is None else self._as_matrix(embeddings)[keep]
        self.upsert([ids[i] for i in keep], embeddings=emb, metadatas=pick(metadatas), documents=pick(documents))

    # ------------------------------------------------------------------ reads
    def get(self, ids: Optional[Sequence[str]] = None, limit: Optional[int] = None, offset: int = 0,
            include: Sequence[str] = ("metadatas", "documents"), where=None, where_document=None) -> dict:
        """chromadb Collection.get: FLAT lists; unknown ids are skipped (store.py:260-261).  `where`: a metadata filter in the
        grammar `query` accepts (one dict); `where_document`: a document filter in the grammar `query` accepts, evaluated on the
        host; with `ids`, the records that satisfy all of them."""
        allowed = None
        if where is not None:
            self._check_where(where)
            allowed = self._where_mask(where)
        if where_document is not None:
            self._check_where_document(where_document)
            in_doc = self._where_document_mask(where_document)
            allowed = in_doc if allowed is None else allowed & in_doc
        if ids is None:
            live = [s for s, doc_id in enumerate(self._ids) if doc_id is not None and (allowed is None or allowed[s])]
            slots = live[offset : (None if limit is None else offset + limit)]
        else:
            slots = [self._slot_of[i] for i in ids if i in self._slot_of and (allowed is None or allowed[self._slot_of[i]])]
        return {
            "ids": [self._ids[s] for s in slots],
            "metadatas": [self._metadatas[s] for s in slots] if "metadatas" in include else None,
            "documents": [self._documents[s] for s in slots] if "documents" in include else None,
            "embeddings": None,
        }

    def query(self, query_texts: Optional[Sequence[str]] = None, query_embeddings=None, n_results: int = 10,
              include: Sequence[str] = ("metadatas", "documents", "distances"), where=None, where_document=None) -> dict:
        """chromadb Collection.query: NESTED lists, one inner list per query, ascending
        distance, min(n_results, count) hits each (store.py:314-329).  `query_texts` are embedded on the engine's device, and stay
        there, when the embedder has embed_on_device, the engine search_tensors and a device, and there are at least
        DEVICE_EMBED_MIN_TEXTS of them; on the host otherwise.  The same vectors either way.

        `where` restricts the search by metadata, in ChromaDB's grammar: {"key": value}, {"key": {"$eq" | "$ne" | "$gt" | "$gte" |
        "$lt" | "$lte": value}}, {"key": {"$in" | "$nin": [values]}}, {"$and" | "$or": [filters]}; as an extension a list of
        filters / None, one per query.  The answer is the exact top-k among the records that satisfy the filter (fewer when
        fewer do; nobody: an empty inner list).  A record without the key fails $eq, $in and the comparisons and passes $ne and
        $nin; a str never compares with a number.  {"namespace": "x"} and {"namespace": {"$eq": "x"}} go through the engine's scoped
        search, every other filter through its masked search (search_masked) under a row mask compiled here; an engine without
        it accepts the namespace forms only.  A malformed filter raises ValueError.

        `where_document` restricts the search by the stored documents, in ChromaDB's grammar: {"$contains": "text"}, {"$not_contains":
        "text"}, {"$and" | "$or": [filters]}; one filter per call, shared by the queries.  Matching is case-sensitive, on the stored
        document's UTF-8 bytes: a substring of code points is a substring of bytes.  A record whose document is None fails $contains
        and passes $not_contains.  Combined with `where`, both must hold.  The answer is the exact top-k among the live records that
        satisfy them (fewer when fewer do; nobody: an empty inner list).  On an engine with match_documents and search_masked_dev
        the needles are matched on the device — the document snapshot is uploaded by the first such call after a change, each
        needle's bitmap is cached (32 entries), $and / $or / $not_contains and a `where` mask are combined there, and one
        search_masked_dev answers; a needle above 256 bytes or holding NUL is evaluated here and uploaded as a mask.  On an engine
        with search_masked only, the filter is evaluated here (`needle in doc`) and goes through search_masked.  An engine with
        neither raises ValueError, as does anything outside the grammar (an empty string, a non-string, an unknown operator).

        On a collection that opted in — metadata "codd:document_regex": 1, or KnnClient(document_regex=True) — the grammar also has
        {"$regex": "pattern"} and {"$not_regex": "pattern"}: the document passes $regex iff re.search(pattern,
        document) finds something, Python's semantics; a record without a document fails $regex and passes $not_regex.  On the
        device path a pattern inside the device subset runs as a byte DFA (match_documents_dfa), plain text as a needle, and
        anything else (back-references, look-around, \\b, flags, Unicode classes on non-ASCII documents) is evaluated here by re
        and uploaded as a mask.  Without the opt-in the two operators are unknown operators, as before.

        On a collection that opted in — metadata "codd:device_where": 1, or KnnClient(device_where=True) — and an engine with
        eval_where, set_column and search_masked_dev, a general `where` is evaluated on the device: the metadata
        of each key a filter names lives there as a column (built by the first such filter, kept up to date by upsert and
        compact, dropped by a load), the filter runs as a predicate program (eval_where), its bitmap is cached (32 entries, until
        the next write), is ANDed with the document bitmap there, and search_masked_dev answers.  The same ids and distances.  A
        filter the device cannot take — a value or literal that is NaN or an int float64 does not hold, more than 32 leaves, 256
        literals or 32 keys — runs on the host as before."""
        if (query_texts is None) == (query_embeddings is None):
            raise ValueError("give exactly one of query_texts / query_embeddings")
        if where_document is not None:
            self._check_where_document(where_document)
        if n_results < 1:
            raise ValueError("n_results must be >= 1")
        if query_embeddings is None:
            if isinstance(query_texts, str):
                query_texts = [query_texts]
            query_texts = list(query_texts)
            if self._embeds_on_device(self._engine, "search_tensors", len(query_texts)):
                q = self._embed.embed_on_device(query_texts, self._engine.device)   # (stays a device tensor: the engine takes it as it is)
            else:
                q = self._as_matrix(self._embed(query_texts))
        else:
            q = self._as_matrix(query_embeddings)
        B = q.shape[0]
        empty = {"ids": [[] for _ in range(B)], "distances": [[] for _ in range(B)] if "distances" in include else None,
                 "metadatas": [[] for _ in range(B)] if "metadatas" in include else None,
                 "documents": [[] for _ in range(B)] if "documents" in include else None, "embeddings": None}
        if self._engine is None or len(self._slot_of) == 0 or B == 0:
            return empty
        if q.shape[1] != self._engine.dim:
            raise ValueError(f"query dimension {q.shape[1]} does not match collection dimension {self._engine.dim}")
        k = min(int(n_results), len(self._slot_of))  # (the live count: deleted records are never returned)
        general = None if where_document is not None else self._general_wheres(where, B)  # (None: nothing but namespace forms, the scoped path below)
        scopes = None if where is None or general is not None or where_document is not None else self._where_scopes(where, B)
        if where_document is not None:
            dist, rows = self._search_by_document(q, k, where_document, where)
        elif general is not None:
            dist, rows = self._search_by_filter(q, k, general)
        elif scopes is None:
            dist, rows = self._engine.search(q, k)
        else:
            if not hasattr(self._engine, "search_scoped"):
                raise NotImplementedError(f"{type(self._engine).__name__} has no scoped search: `where` needs an engine with search_scoped")
            known = scopes >= 0
            dist = np.full((B, k), np.inf, dtype=np.float32)
            rows = np.full((B, k), -1, dtype=np.int64)
            if known.any():
                dist[known], rows[known] = self._engine.search_scoped(self._rows_of(q, known), scopes[known].astype(np.uint32), k)
        out = empty
        for b in range(B):
            hit = [(int(r), float(d)) for r, d in zip(rows[b].tolist(), dist[b].tolist()) if r >= 0]
            out["ids"][b] = [self._ids[r] for r, _ in hit]
            if out["distances"] is not None:
                out["distances"][b] = [d for _, d in hit]
            if out["metadatas"] is not None:
                out["metadatas"][b] = [self._metadatas[r] for r, _ in hit]
            if out["documents"] is not None:
                out["documents"][b] = [self._documents[r] for r, _ in hit]
        return out


    def _general_wheres(self, where, B: int) -> Optional[list]:
        """None when every query's filter is None or a namespace form (the scoped path, as before).  Otherwise the per-query filters,
        each checked against the grammar; needs an engine with search_masked, else the ValueError that names the namespace forms."""
        if where is None:
            return None
        if isinstance(where, (list, tuple)):
            if len(where) != B:
                return None  # (_where_scopes raises the length error)
            per_query = list(where)
        else:
            per_query = [where] * B
        found = False
        for w in per_query:
            try:
                self._where_namespace(w)
            except ValueError:
                found = True
        if not found:
            return None
        if not hasattr(self._engine, "search_masked"):
            bad = next(w for w in per_query if not self._is_namespace_form(w))
            raise ValueError(f"unsupported where filter {bad!r}; supported: {self._WHERE_FORMS}")
        for w in per_query:
            if w is not None and not self._is_namespace_form(w):
                self._check_where(w)
        return per_query

    @classmethod
    def _is_namespace_form(cls, where) -> bool:
        try:
            cls._where_namespace(where)
            return True
        except ValueError:
            return False

    def _search_by_filter(self, q, k: int, per_query: list):
        """One engine call per group of queries with the same filter: None -> search, a namespace form -> search_scoped, each distinct
        general filter -> search_masked under its compiled mask (no call when nobody matches: that query's hits stay empty)."""
        B = q.shape[0]
        dist = np.full((B, k), np.inf, dtype=np.float32)
        rows = np.full((B, k), -1, dtype=np.int64)
        plain = [b for b, w in enumerate(per_query) if w is None]
        scoped = [b for b, w in enumerate(per_query) if w is not None and self._is_namespace_form(w)]
        if plain:
            dist[plain], rows[plain] = self._engine.search(self._rows_of(q, plain), k)
        if scoped:
            if not hasattr(self._engine, "search_scoped"):
                raise NotImplementedError(f"{type(self._engine).__name__} has no scoped search: `where` needs an engine with search_scoped")
            labels = np.array([self._scope_of_namespace.get(self._where_namespace(per_query[b]), -1) for b in scoped], dtype=np.int64)
            known = [b for b, s in zip(scoped, labels.tolist()) if s >= 0]
            if known:
                dist[known], rows[known] = self._engine.search_scoped(self._rows_of(q, known), labels[labels >= 0].astype(np.uint32), k)
        groups: dict[str, list[int]] = {}
        for b, w in enumerate(per_query):
            if w is not None and not self._is_namespace_form(w):
                groups.setdefault(json.dumps(w, sort_keys=True, ensure_ascii=False), []).append(b)
        for members in groups.values():
            # opted in: the filter's bitmap is made, and stays, on the device; search_masked_dev counts it there
            bits = self._where_bits(per_query[members[0]]) if self._has_device_where() else None
            if bits is not None:
                dist[members], rows[members] = self._engine.search_masked_dev(self._rows_of(q, members), bits, k)
                continue
            mask = self._where_mask(per_query[members[0]])
            if mask.any():
                dist[members], rows[members] = self._engine.search_masked(self._rows_of(q, members), mask, k)
        return dist, rows

    def _search_by_document(self, q, k: int, where_document, where):
        """The exact top-k among the live records that satisfy `where_document` and, per query, `where` (None, a namespace form or a
        general filter; one for all queries or a list): one masked engine call per distinct `where`."""
        B = q.shape[0]
        if not hasattr(self._engine, "search_masked"):
            raise ValueError(f"unsupported where_document filter {where_document!r}: {type(self._engine).__name__} has no masked search; "
                             f"supported on an engine with search_masked: {self._WHERE_DOCUMENT_GRAMMAR}")
        if isinstance(where, (list, tuple)):
            if len(where) != B:
                raise ValueError(f"where has {len(where)} entries for {B} queries; supported: {self._WHERE_FORMS}")
            per_query = list(where)
        else:
            per_query = [where] * B
        groups: dict[str, list[int]] = {}
        for b, w in enumerate(per_query):
            if w is not None:
                self._check_where(w)   # (the namespace forms are filters of the general grammar too)
            groups.setdefault(json.dumps(w, sort_keys=True, ensure_ascii=False), []).append(b)
        dist = np.full((B, k), np.inf, dtype=np.float32)
        rows = np.full((B, k), -1, dtype=np.int64)
        on_device = self._has_device_documents() and self._documents_fit_device()
        for members in groups.values():
            w = per_query[members[0]]
            where_bits = self._where_bits(w) if w is not None and on_device and self._has_device_where() else None
            if where_bits is not None:   # (opted in, DESIGN.md §26: both bitmaps are on the device already, nothing is uploaded)
                bits = self._where_document_bits(where_document) & where_bits
                dist[members], rows[members] = self._engine.search_masked_dev(self._rows_of(q, members), bits, k)
                continue
            by_where = None if w is None else self._where_mask(w)
            if by_where is not None and not by_where.any():
                continue
            if on_device:
                bits = self._where_document_bits(where_document)
                if by_where is not None:
                    bits = bits & self._words_on_device(by_where)
                dist[members], rows[members] = self._engine.search_masked_dev(self._rows_of(q, members), bits, k)
            else:
                mask = self._where_document_mask(where_document)
                if by_where is not None:
                    mask = mask & by_where
                if mask.any():
                    dist[members], rows[members] = self._engine.search_masked(self._rows_of(q, members), mask, k)
        return dist, rows

    # ------------------------------------------------------------------ persistence
    def _write_generation(self, directory: str) -> None:
        """Write gen-<n+1> under `directory`, then flip CURRENT (atomic rename)."""
        self.compact()  # a generation on disk holds live rows only (the format knows nothing of tombstones)
        gen = self._generation + 1
        name = f"gen-{gen:08d}"
        tmp = os.path.join(directory, f".{name}.tmp-{os.getpid()}")
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp)
        n = len(self._ids)
        manifest = {"format_version": FORMAT_VERSION, "name": self.name, "metadata": self.metadata, "count": n,
                    "dim": None, "padded_dim": None, "dtype": None}
        if self._engine is not None and n:
            rows = self._engine.read_rows(0, n)
            manifest.update(dim=self._engine.dim, padded_dim=int(rows.shape[1]), dtype=getattr(self._engine, "dtype", "f32"))
            # whether every stored row is a unit vector: both MFMA filters assume it, and a reader of this generation has no
            # other way to know that some rows were written with normalize = 0 (its own norm check of rows.bin comes on top)
            stat = getattr(self._engine, "stat", None)
            manifest["all_normalized"] = bool(stat("all_normalized")) if callable(stat) else True
            rows.tofile(os.path.join(tmp, "rows.bin"))
        with open(os.path.join(tmp, "ids.json"), "w") as f:
            json.dump(self._ids, f, ensure_ascii=False)
        for fname, seq in (("metadatas.jsonl", self._metadatas), ("documents.jsonl", self._documents)):
            with open(os.path.join(tmp, fname), "w") as f:
                for item in seq:
                    f.write(json.dumps(item, ensure_ascii=False) + "\n")
        with open(os.path.join(tmp, "manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1, ensure_ascii=False)
        final = os.path.join(directory, name)
        shutil.rmtree(final, ignore_errors=True)
        os.replace(tmp, final)
        cur_tmp = os.path.join(directory, f".CURRENT.tmp-{os.getpid()}")
        with open(cur_tmp, "w") as f:
            f.write(name)
        os.replace(cur_tmp, os.path.join(directory, "CURRENT"))
        for old in os.listdir(directory):  # keep the previous generation for a reader that is mid-load
            if old.startswith("gen-") and old not in (name, f"gen-{gen - 1:08d}"):
                shutil.rmtree(os.path.join(directory, old), ignore_errors=True)
        self._generation = gen
        self._dirty = False

    @staticmethod
    def _current_generation(directory: str) -> Optional[str]:
        try:
            with open(os.path.join(directory, "CURRENT")) as f:
                return f.read().strip() or None
        except OSError:
            return None

    def _load_generation(self, directory: str, gen_name: str) -> None:
        gdir = os.path.join(directory, gen_name)
        with open(os.path.join(gdir, "manifest.json")) as f:
            manifest = json.load(f)
        if manifest.get("format_version") != FORMAT_VERSION:
            raise ValueError(f"{gdir}: unsupported index format {manifest.get('format_version')}")
        with open(os.path.join(gdir, "ids.json")) as f:
            ids = json.load(f)
        read_lines = lambda fname: [json.loads(line) for line in open(os.path.join(gdir, fname))]  # noqa: E731
        metadatas, documents = read_lines("metadatas.jsonl"), read_lines("documents.jsonl")
        n = manifest["count"]
        if not (len(ids) == len(metadatas) == len(documents) == n):
            raise ValueError(f"{gdir}: sidecar lengths disagree with the manifest")
        # the space travels in the stored collection metadata; an engine this collection already has must be of that space
        space = _space_of(manifest.get("metadata"))
        if self._engine is not None and getattr(self._engine, "space", _DEFAULT_SPACE) != space:
            raise ValueError(f"{gdir}: stored space {space} does not match the collection's space {getattr(self._engine, 'space', _DEFAULT_SPACE)}")
        engine = None
        if n and manifest["dim"]:
            dtype = manifest["dtype"]
            rows = np.fromfile(os.path.join(gdir, "rows.bin"), dtype=np.float32 if dtype == "f32" else np.uint16)
            rows = rows.reshape(n, manifest["padded_dim"])
            engine = self._make_engine(manifest["dim"], space, manifest.get("metadata") or {})
            if getattr(engine, "dtype", dtype) != dtype:
                raise ValueError(f"{gdir}: stored dtype {dtype} does not match the client's dtype {engine.dtype}")
            engine.load_rows(rows, 0)
            if manifest.get("all_normalized") is False and callable(getattr(engine, "set_option", None)):
                engine.set_option("all_normalized", 0)
        old = self._engine
        self._engine = engine
        if old is not None and hasattr(old, "close"):
            old.close()
        self._columns.clear()   # (derived data of the rows that were: the new engine holds no column, nothing of them is on disk)
        self.metadata = dict(manifest.get("metadata") or {})
        self._ids, self._metadatas, self._documents = ids, metadatas, documents
        self._slot_of = {doc_id: i for i, doc_id in enumerate(ids)}
        self._forget_where_index()
        # namespaces -> scope labels, from the stored metadata (the on-disk format knows nothing of scopes)
        self._scope_of_namespace = {}
        scopes = np.array([self._scope_for(md) for md in metadatas], dtype=np.uint32)
        if engine is not None and scopes.any() and hasattr(engine, "set_scopes"):
            engine.set_scopes(np.arange(n, dtype=np.int64), scopes)
        self._generation = int(gen_name.split("-")[1])
        self._dirty = False


class KnnClient:
    """Stands where `chromadb.HttpClient(host, port)` / `EphemeralClient()` stand.

    Args:
        device: GPU that holds the row stores ("cuda:0").
        dtype: storage dtype of the rows: "f32" | "bf16" | "f16".
        embedding_function: list[str] -> [n,d] float32; default HashingEmbeddingFunction(384).
        engine_factory: test seam, see module docstring.
        document_regex: every collection of this client answers `where_document` {"$regex": ...} / {"$not_regex": ...} (DESIGN.md
            §24); without it only a collection whose metadata carries "codd:document_regex": 1 does.
        device_where: every collection of this client evaluates a general `where` on the engine's device (metadata
            columns and a predicate kernel; the same answers); without it only a collection whose metadata carries
            "codd:device_where": 1 does.
    """

    def __init__(self, device: str = "cuda:0", dtype: str = "f32", embedding_function: Optional[EmbeddingFunction] = None,
                 engine_factory: Optional[Callable[[int], Any]] = None, path: Optional[str] = None, document_regex: bool = False,
                 device_where: bool = False):
        self.device = device
        self.document_regex = bool(document_regex)
        self.device_where = bool(device_where)
        self.dtype = dtype
        self.path = path
        self._embed = embedding_function or HashingEmbeddingFunction()
        self._engine_factory = engine_factory or _default_engine_factory(device, dtype)
        self._collections: dict[str, Collection] = {}
        if path is not None:
            os.makedirs(path, exist_ok=True)
            for entry in sorted(os.listdir(path)):
                cdir = os.path.join(path, entry)
                gen = Collection._current_generation(cdir) if os.path.isdir(cdir) else None
                if gen:
                    col = Collection(entry, None, self._embed, self._engine_factory, self.document_regex, self.device_where)
                    col._load_generation(cdir, gen)
                    self._collections[col.name] = col

    # ------------------------------------------------------------------ persistence
    def _dir_of(self, name: str) -> str:
        if os.sep in name or name.startswith("."):
            raise ValueError(f"collection name {name!r} cannot be used as a directory name")
        return os.path.join(self.path, name)

    def persist(self) -> int:
        """Write every changed collection to `path` (new generation + CURRENT flip). Returns how many."""
        if self.path is None:
            return 0
        written = 0
        for col in self._collections.values():
            if col._dirty or col._generation == 0:
                cdir = self._dir_of(col.name)
                os.makedirs(cdir, exist_ok=True)
                col._write_generation(cdir)
                written += 1
        return written

    def reload(self) -> int:
        """Pick up generations another process (the indexer job) has published since we loaded."""
        if self.path is None:
            return 0
        loaded = 0
        for entry in sorted(os.listdir(self.path)):
            cdir = os.path.join(self.path, entry)
            gen = Collection._current_generation(cdir) if os.path.isdir(cdir) else None
            if not gen:
                continue
            col = self._collections.get(entry)
            if col is None:
                col = Collection(entry, None, self._embed, self._engine_factory, self.document_regex, self.device_where)
                self._collections[entry] = col
            if int(gen.split("-")[1]) > col._generation:
                col._load_generation(cdir, gen)
                loaded += 1
        return loaded

    def heartbeat(self) -> int:
        """Liveness probe (indexer_main.py:215,330): nanoseconds since the epoch, like chromadb."""
        return time.time_ns()

    def get_or_create_collection(self, name: str, metadata: Optional[dict] = None,
                                 embedding_function: Optional[EmbeddingFunction] = None) -> Collection:
        if not isinstance(name, str) or not name:
            raise ValueError("collection name must be a non-empty string")
        existing = self._collections.get(name)
        if existing is not None:
            return existing
        space = _space_of(metadata)
        if space not in _factory_spaces(self._engine_factory):
            raise ValueError(f"hnsw:space={space!r} is not on this path (supported: {_factory_spaces(self._engine_factory)})")
        col = Collection(name, metadata, embedding_function or self._embed, self._engine_factory, self.document_regex, self.device_where)
        self._collections[name] = col
        return col

    def create_collection(self, name: str, metadata: Optional[dict] = None, embedding_function=None) -> Collection:
        if name in self._collections:
            raise ValueError(f"Collection {name} already exists")
        return self.get_or_create_collection(name, metadata, embedding_function)

    def get_collection(self, name: str) -> Collection:
        try:
            return self._collections[name]
        except KeyError:
            raise ValueError(f"Collection {name} does not exist") from None

    def list_collections(self) -> list[str]:
        return list(self._collections)

    def delete_collection(self, name: str) -> None:
        col = self._collections.pop(name, None)
        if col is None:
            raise ValueError(f"Collection {name} does not exist")
        eng = col._engine
        if eng is not None and hasattr(eng, "close"):
            eng.close()
        if self.path is not None:
            shutil.rmtree(self._dir_of(name), ignore_errors=True)
