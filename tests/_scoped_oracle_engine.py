"""OracleEngine with scopes, for the host-logic tests of namespace-scoped search: a scoped search over scope s is the
oracle's search over the sub-matrix of the rows whose scope is s (row order kept, so "ties -> lower row" carries over), its
indices mapped back through np.flatnonzero.  Scope 0 in a query means every row."""

from __future__ import annotations

import numpy as np

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests._oracle_engine import OracleEngine


def scoped_reference(rows: np.ndarray, dtype: str, scope_of: np.ndarray, qn: np.ndarray, scopes, k: int):
    """(dist [B,k], rows [B,k]) of normalised queries qn restricted per query to scopes[b]; +inf / -1 padded."""
    B = qn.shape[0]
    dist = np.full((B, k), np.inf, dtype=np.float32)
    idx = np.full((B, k), -1, dtype=np.int64)
    for b, s in enumerate(np.asarray(scopes).tolist()):
        members = np.arange(rows.shape[0]) if s == 0 else np.flatnonzero(scope_of[: rows.shape[0]] == s)
        if members.size == 0:
            continue
        d, i = o.search(np.ascontiguousarray(rows[members]), dtype, qn[b : b + 1], k)
        hit = i[0] >= 0
        dist[b, hit] = d[0][hit]
        idx[b, hit] = members[i[0][hit]]
    return dist, idx


class ScopedOracleEngine(OracleEngine):
    def __init__(self, dim: int, dtype: str = "f32"):
        super().__init__(dim, dtype)
        self._scope_of = np.zeros(0, dtype=np.uint32)
        self.calls: list[str] = []

    def _labels(self) -> np.ndarray:
        if self._scope_of.shape[0] < self.count():  # a new slot starts with scope 0
            self._scope_of = np.concatenate([self._scope_of, np.zeros(self.count() - self._scope_of.shape[0], dtype=np.uint32)])
        return self._scope_of

    def set_scopes(self, slots, scopes) -> None:
        slots = np.asarray(slots, dtype=np.int64)
        scopes = np.asarray(scopes, dtype=np.uint32)
        assert slots.shape == scopes.shape and (slots.size == 0 or (slots.min() >= 0 and slots.max() < self.count()))
        self.calls.append("set_scopes")
        self._labels()[slots] = scopes

    def search_scoped(self, queries, scopes, k: int):
        self.calls.append("search_scoped")
        return scoped_reference(self._rows, self.dtype, self._labels(), self._prep(queries), scopes, k)

    def search(self, queries, k: int):
        self.calls.append("search")
        return super().search(queries, k)

    def search_keys_scoped(self, queries, scopes, k: int, row_base: int = 0) -> np.ndarray:
        row_base = native.check_row_base(row_base, self.count())
        qn = self._prep(queries)
        keys = np.zeros((qn.shape[0], k), dtype=np.uint64)
        labels = self._labels()
        for b, s in enumerate(np.asarray(scopes).tolist()):
            members = np.arange(self.count()) if s == 0 else np.flatnonzero(labels == s)
            if members.size == 0:
                continue
            # keys of the sub-matrix carry sub-matrix indices: unpack, map back, repack with the global row
            sub = o.search_keys(np.ascontiguousarray(self._rows[members]), self.dtype, qn[b : b + 1], k, 0)[0]
            live = sub != 0
            local = (np.uint64(0xFFFFFFFF) - (sub[live] & np.uint64(0xFFFFFFFF))).astype(np.int64)
            rows = (members[local] + row_base).astype(np.uint64)
            keys[b, live] = (sub[live] & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - rows)
        return keys
