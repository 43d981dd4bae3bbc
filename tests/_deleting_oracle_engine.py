"""ScopedOracleEngine with tombstones, for the host-logic tests of Collection.delete: a search is the oracle's search over
the sub-matrix of the LIVE rows (row order kept, so "ties -> lower row" carries over), its indices mapped back to row slots
through the monotone map np.flatnonzero(live).  compact() is the stable squeeze the engine's contract states: live rows to
slots 0 .. live-1 in slot order, scopes along with them.  A dead slot cannot be written until then."""

from __future__ import annotations

import numpy as np

from oracle import knn_oracle as o
from tests._scoped_oracle_engine import ScopedOracleEngine


def live_reference(rows: np.ndarray, dtype: str, live_slots: np.ndarray, qn: np.ndarray, k: int):
    """(dist [B,k], rows [B,k]) of normalised queries qn over the rows at `live_slots` (ascending); +inf / -1 padded."""
    B = qn.shape[0]
    dist = np.full((B, k), np.inf, dtype=np.float32)
    idx = np.full((B, k), -1, dtype=np.int64)
    if live_slots.size:
        d, i = o.search(np.ascontiguousarray(rows[live_slots]), dtype, qn, k)
        hit = i >= 0
        dist[hit] = d[hit]
        idx[hit] = live_slots[i[hit]]
    return dist, idx


class DeletingOracleEngine(ScopedOracleEngine):
    def __init__(self, dim: int, dtype: str = "f32"):
        super().__init__(dim, dtype)
        self._dead = np.zeros(0, dtype=bool)
        self.compactions = 0

    def _dead_mask(self) -> np.ndarray:
        if self._dead.shape[0] < self.count():
            self._dead = np.concatenate([self._dead, np.zeros(self.count() - self._dead.shape[0], dtype=bool)])
        return self._dead

    def _live_slots(self) -> np.ndarray:
        return np.flatnonzero(~self._dead_mask()[: self.count()])

    # ---- writes: a dead slot stays dead until compact()
    def _check_writable(self, slots) -> None:
        slots = np.asarray(slots, dtype=np.int64)
        old = slots[slots < self._dead_mask().shape[0]]
        if old.size and self._dead[old].any():
            raise ValueError("write into a dead slot")

    def upsert(self, slots, vecs, normalize: bool = True) -> None:
        self._check_writable(slots)
        super().upsert(slots, vecs, normalize)

    def set_scopes(self, slots, scopes) -> None:
        self._check_writable(slots)
        super().set_scopes(slots, scopes)

    # ---- the three calls of the engine protocol
    def delete(self, slots) -> None:
        slots = np.asarray(slots, dtype=np.int64)
        if slots.size and (slots.min() < 0 or slots.max() >= self.count()):
            raise ValueError("delete: row slot outside [0, count)")
        self.calls.append("delete")
        self._dead_mask()[slots] = True

    def live_count(self) -> int:
        return int(self._live_slots().size)

    def compact(self) -> int:
        self.calls.append("compact")
        live = self._live_slots()
        if live.size != self.count():
            self.compactions += 1
            self._scope_of = self._labels()[live].copy()
            self._rows = np.ascontiguousarray(self._rows[live])
            self._dead = np.zeros(live.size, dtype=bool)
        return self.count()

    # ---- searches: the oracle over the live rows, slots mapped back
    def search(self, queries, k: int):
        self.calls.append("search")
        return live_reference(self._rows, self.dtype, self._live_slots(), self._prep(queries), k)

    def search_scoped(self, queries, scopes, k: int):
        self.calls.append("search_scoped")
        qn = self._prep(queries)
        labels, dead = self._labels(), self._dead_mask()
        B = qn.shape[0]
        dist = np.full((B, k), np.inf, dtype=np.float32)
        idx = np.full((B, k), -1, dtype=np.int64)
        for b, s in enumerate(np.asarray(scopes).tolist()):
            member = ~dead[: self.count()] if s == 0 else (labels[: self.count()] == s) & ~dead[: self.count()]
            dist[b : b + 1], idx[b : b + 1] = live_reference(self._rows, self.dtype, np.flatnonzero(member), qn[b : b + 1], k)
        return dist, idx
