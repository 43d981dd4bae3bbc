"""MaskedOracleEngine with ChromaDB's spaces, for the host-logic tests of l2 and ip collections: under "cosine" it
is its parent; under "l2" / "ip" every search is tests/_space_reference.Reference over the rows that are live (and in the scope, and
allowed).  `factory(dtype)` is an engine factory as KnnClient takes one, with the `spaces` attribute that says it builds them."""

from __future__ import annotations

import numpy as np

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _space_reference as sr
from tests._masked_oracle_engine import MaskedOracleEngine, allowed_rows


class SpaceOracleEngine(MaskedOracleEngine):
    def __init__(self, dim: int, dtype: str = "f32", space: str = "cosine"):
        super().__init__(dim, dtype)
        native.metric_code(space)
        self.space = space
        self.normalize_args: list[bool] = []   # the `normalize` of every upsert

    def upsert(self, slots, vecs, normalize: bool = True) -> None:
        self.normalize_args.append(bool(normalize))
        if self.space == "cosine" or normalize:
            return super().upsert(slots, vecs, normalize)
        # as the engine stores them under ip / l2: non-finite and all-zero vectors as zeros, nothing normalised
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        super().upsert(slots, sr.clean(vecs, self.padded_dim)[:, : self.dim], False)

    def _answer(self, queries, k: int, member: np.ndarray, per_query=None):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        ref = sr.Reference(self.space, None, self.dtype, q, rows_storage=self._rows)
        if per_query is None:
            _, dist, rows = ref.topk(q.shape[0], k, allow=member)
            return dist, rows
        dist = np.full((q.shape[0], k), np.inf, dtype=np.float32)
        rows = np.full((q.shape[0], k), -1, dtype=np.int64)
        for b, m in enumerate(per_query):
            _, dist[b : b + 1], rows[b : b + 1] = ref.topk(1, k, allow=m, queries=[b])
        return dist, rows

    def _live(self) -> np.ndarray:
        return ~self._dead_mask()[: self.count()]

    def search(self, queries, k: int):
        if self.space == "cosine":
            return super().search(queries, k)
        self.calls.append("search")
        return self._answer(queries, k, self._live())

    def search_scoped(self, queries, scopes, k: int):
        if self.space == "cosine":
            return super().search_scoped(queries, scopes, k)
        self.calls.append("search_scoped")
        labels, live = self._labels()[: self.count()], self._live()
        return self._answer(queries, k, None, [live if s == 0 else live & (labels == s) for s in np.asarray(scopes).tolist()])

    def search_masked(self, queries, allow, k: int):
        if self.space == "cosine":
            return super().search_masked(queries, allow, k)
        self.calls.append("search_masked")
        member = allowed_rows(allow, self.count())
        self.masks.append(member.copy())
        return self._answer(queries, k, member & self._live())

    def search_keys(self, queries, k: int, row_base: int = 0) -> np.ndarray:
        if self.space == "cosine":
            return super().search_keys(queries, k, row_base)
        row_base = native.check_row_base(row_base, self.count())
        q = np.ascontiguousarray(queries, dtype=np.float32)
        return sr.Reference(self.space, None, self.dtype, q, rows_storage=self._rows).topk(q.shape[0], k, allow=self._live(), row_base=row_base)[0]

    def merge_keys(self, keys: np.ndarray, k: int):
        """the shard merge of this engine's space: the integer top-k, distances by the space"""
        merged = o.merge_keys(keys, k)
        if self.space == "cosine":
            dist, rows = o.unpack_keys(merged)
            return merged, dist, rows
        rows = sr.key_rows(merged)
        return merged, sr.distances(self.space, sr.key_scores(merged), rows >= 0), rows


def factory(dtype: str = "f32", made: list | None = None):
    """engine_factory for KnnClient that builds every space; `made` collects the engines it built"""
    def make(dim: int, space: str = "cosine"):
        eng = SpaceOracleEngine(dim, dtype, space)
        if made is not None:
            made.append(eng)
        return eng

    make.spaces = ("cosine", "l2", "ip")
    return make
