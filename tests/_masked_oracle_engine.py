"""DeletingOracleEngine with search_masked, for the host-logic tests of a general `where`: a masked search is the
oracle's search over the sub-matrix of the rows that are allowed AND live (row order kept, so "ties -> lower row" carries over),
its indices mapped back to row slots.  The mask arrives as the engine protocol states it: a bool array of length count(), or packed
uint32 words (bit r & 31 of word r >> 5 = row slot r)."""

from __future__ import annotations

import numpy as np

from tests._deleting_oracle_engine import DeletingOracleEngine, live_reference


def allowed_rows(allow, count: int) -> np.ndarray:
    """bool [count] from either form of the mask; bits at or above count are ignored."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        assert a.shape == (count,), (a.shape, count)
        return a
    assert a.dtype == np.uint32 and a.shape == ((count + 31) // 32,), (a.dtype, a.shape, count)
    return np.unpackbits(a.view(np.uint8), bitorder="little")[:count].astype(bool)


class MaskedOracleEngine(DeletingOracleEngine):
    def __init__(self, dim: int, dtype: str = "f32"):
        super().__init__(dim, dtype)
        self.masks: list[np.ndarray] = []   # the mask of every search_masked call, as bool [count]

    def search_masked(self, queries, allow, k: int):
        self.calls.append("search_masked")
        n = self.count()
        member = allowed_rows(allow, n)
        self.masks.append(member.copy())
        return live_reference(self._rows, self.dtype, np.flatnonzero(member & ~self._dead_mask()[:n]), self._prep(queries), k)
