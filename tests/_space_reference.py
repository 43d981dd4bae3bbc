"""CPU restatement of the ip and l2 spaces, bit for bit what the engine must return.

The contract (ChromaDB's definitions)
    rows and queries are used as given: padded with zeros to the stored width, never normalised; a vector with a NaN or infinite
    element, or without a non-zero one, is the zero vector; rows are then rounded to the storage dtype (o.to_storage / o.widen)
    ip   score = the canonical dot product of DESIGN.md §3 (o.search_keys on the unnormalised operands), distance = 1 - score in fp32
    l2   distance = o.canon_dot(d, d) with d = q - widen(c) computed in numpy fp32 (one IEEE subtraction per element), the chunk
         width of the storage dtype; the score a key carries is 0.0f - distance.  Ordered by (distance, row).
    ties -> lower row; padding: row -1, distance +inf, key 0

Keys are (ord(score) << 32) | (0xFFFFFFFF - global row) with the order map of DESIGN.md §2, restated here with its inverse:
    ord(s)  = ~bits(s) if the sign bit is set, else bits(s) | 0x80000000        (a NaN score ranks as -inf)
    ord^-1  : o & 0x7FFFFFFF if o has the top bit, else ~o
"""

from __future__ import annotations

import ctypes

import numpy as np

from oracle import knn_oracle as o

SPACES = ("l2", "ip")


def clean(x: np.ndarray, dpad: int | None = None) -> np.ndarray:
    """fp32 [n, d] -> fp32 [n, dpad]: zero padded; rows with a non-finite element or without a non-zero one are all zeros"""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    dpad = o.pad_dim(d) if dpad is None else dpad
    out = np.zeros((n, dpad), dtype=np.float32)
    good = np.isfinite(x).all(axis=1) & (x != 0).any(axis=1)
    out[good, :d] = x[good]
    return out


def stored(raw: np.ndarray, dtype: str) -> np.ndarray:
    """the rows as an ip / l2 index of `dtype` stores them (what read_rows returns): fp32, or uint16 bit patterns"""
    return o.to_storage(clean(raw), dtype)


def ord_f32(s: np.ndarray) -> np.ndarray:
    s = np.asarray(s, dtype=np.float32).copy()
    s[np.isnan(s)] = -np.inf
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unord_f32(hi: np.ndarray) -> np.ndarray:
    hi = np.asarray(hi, dtype=np.uint32)
    return np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32).view(np.float32)


def make_keys(score: np.ndarray, rows: np.ndarray, row_base: int = 0) -> np.ndarray:
    """packed keys of (fp32 score, local row) pairs; row < 0 -> 0 (empty)"""
    rows = np.asarray(rows, dtype=np.int64)
    low = (np.int64(0xFFFFFFFF) - (rows + row_base)).astype(np.uint64)
    keys = (ord_f32(score).astype(np.uint64) << np.uint64(32)) | low
    return np.where(rows >= 0, keys, np.uint64(0))


def key_scores(keys: np.ndarray) -> np.ndarray:
    return unord_f32((np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32))


def key_rows(keys: np.ndarray, row_base: int = 0) -> np.ndarray:
    keys = np.asarray(keys, dtype=np.uint64)
    rows = np.int64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64) - row_base
    return np.where(keys != 0, rows, -1)


def distances(space: str, score: np.ndarray, have: np.ndarray) -> np.ndarray:
    """the fp32 distance beside a key's score: 1 - s (ip), 0 - s (l2); +inf where no row"""
    one = np.float32(1.0 if space == "ip" else 0.0)
    with np.errstate(invalid="ignore"):
        return np.where(have, one - np.asarray(score, dtype=np.float32), np.float32(np.inf)).astype(np.float32)


def l2_matrix(rows_storage: np.ndarray, dtype: str, q_clean: np.ndarray) -> np.ndarray:
    """[B, n] fp32 canonical squared distances: canon_dot(d, d) of d = q - widen(c) per pair"""
    W = o.widen(rows_storage, dtype)
    B, (n, dpad) = q_clean.shape[0], W.shape
    E = o.lib().oracle_elems_per_chunk(o._DT_BY_NAME[dtype])
    fn = o.lib().oracle_canon_dot
    out = np.empty((B, n), dtype=np.float32)
    for b in range(B):
        D = np.ascontiguousarray(q_clean[b][None, :] - W, dtype=np.float32)   # one IEEE fp32 subtraction per element
        base, step = D.ctypes.data, dpad * 4
        out[b] = [fn(ctypes.c_void_p(base + i * step), ctypes.c_void_p(base + i * step), dpad, E) for i in range(n)]
    return out + np.float32(0.0)


class Reference:
    """The answers of one index (raw rows, storage dtype, space) to one block of raw queries, any prefix of it, any k, any row
    mask.  The l2 distance matrix is computed once and shared by every call."""

    def __init__(self, space: str, raw_rows: np.ndarray, dtype: str, raw_queries: np.ndarray, rows_storage: np.ndarray | None = None):
        assert space in SPACES
        self.space, self.dtype = space, dtype
        self.rows = stored(raw_rows, dtype) if rows_storage is None else rows_storage
        self.q = clean(raw_queries, self.rows.shape[1])
        self.n = self.rows.shape[0]
        self._l2 = None

    def l2(self) -> np.ndarray:
        if self._l2 is None:
            self._l2 = l2_matrix(self.rows, self.dtype, self.q)
        return self._l2

    def topk(self, B: int, k: int, allow: np.ndarray | None = None, row_base: int = 0, queries: np.ndarray | None = None):
        """(keys u64 [B, k], dist fp32 [B, k], rows int64 [B, k]) of the first B queries (or of the query numbers `queries`) among
        the rows `allow` names (bool [n]; None = all)."""
        qsel = np.arange(B) if queries is None else np.asarray(queries)
        idx = np.arange(self.n) if allow is None else np.flatnonzero(np.asarray(allow, dtype=bool)[: self.n])
        score = np.zeros((len(qsel), k), dtype=np.float32)
        rows = np.full((len(qsel), k), -1, dtype=np.int64)
        if idx.size:
            if self.space == "ip":
                sub = o.search_keys(np.ascontiguousarray(self.rows[idx]), self.dtype, np.ascontiguousarray(self.q[qsel]), k)
                have = sub != 0
                score = np.where(have, key_scores(sub), np.float32(0.0)).astype(np.float32)
                rows = np.where(have, idx[np.where(have, key_rows(sub), 0)], -1)
            else:
                D = self.l2()[np.ix_(qsel, idx)]
                kk = min(k, idx.size)
                order = np.lexsort((np.broadcast_to(idx, D.shape), D), axis=1)[:, :kk]
                rows[:, :kk] = idx[order]
                score[:, :kk] = np.float32(0.0) - np.take_along_axis(D, order, axis=1)
        have = rows >= 0
        return make_keys(score, rows, row_base), distances(self.space, score, have), rows


def brute64(space: str, rows_f32: np.ndarray, q: np.ndarray) -> np.ndarray:
    """[B, n] fp64 distances of ChromaDB's definitions over already stored (widened) rows: the same arithmetic, wider"""
    R, Q = np.asarray(rows_f32, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if space == "ip":
        return 1.0 - Q @ R.T
    return ((Q[:, None, :] - R[None, :, :]) ** 2).sum(axis=2)
