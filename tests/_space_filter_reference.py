"""CPU restatement of the int8 filter leg of an ip or l2 index: the quantisation as the builder and the query
preparation choose it, the measured norms, the filter value of every (query, row) in the fp32 operations of the device, and the
slack eps(q) that the leg puts between that value and the exact score.

    rows     stored rows widened to fp32, padded with zeros to a multiple of 128 elements (the int8 K-step)
    s_blk    one scale per block of 32 rows: fp32(max |c_i| over the block / 127), 1 for a block of zeros; inv = fp32(1 / s_blk);
             c~_i = s_blk * clip(rint(fp32(c_i * inv)), -127, 127)
    e_r      max over rows of fp32(sqrt(sum (c_i - fp32(t_i * s_blk))^2) * 1.0001 + 1e-7)       (the builder's measured norm)
    rn2      the canonical sum of squares of the stored row (oracle canon_dot, the storage dtype's chunk width)
    R        max over rows of fp32(sqrt(rn2) * 1.0001 + 1e-7)
    s_q      fp32(max |q_i| / 127), 0 for the zero query; the query quantised with inv = fp32(127 / max |q_i|)
    n_q      canon_dot(q, q) with chunks of 4;  Q = fp32(sqrt(n_q) * 1.0001 + 1e-7)
    value    ip: fp32(fp32(fp32(acc) * s_blk) * s_q);  l2: fp32(fma(fp32(fp32(acc) * s_blk), 2 s_q, -rn2) - n_q)
    eps(q)   the two formulas of prep_queries8_raw_kernel, evaluated in fp32 in its order
"""

from __future__ import annotations

import ctypes

import numpy as np

from oracle import knn_oracle as o
from tests import _space_reference as sr

f32 = np.float32
UP, U24, U23 = f32(1.0001), f32(2.0**-24), f32(2.0**-23)
BAND_LO, BAND_HI = f32(2.0**-100), f32(2.0**100)


def pad128(x: np.ndarray) -> np.ndarray:
    n, d = x.shape
    out = np.zeros((n, (d + 127) // 128 * 128), dtype=np.float32)
    out[:, :d] = x
    return out


def canon_sq(x: np.ndarray, E: int) -> np.ndarray:
    """canonical sum of squares of every fp32 row of x (width a multiple of 64)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fn = o.lib().oracle_canon_dot
    base, step, w = x.ctypes.data, x.shape[1] * 4, x.shape[1]
    with np.errstate(over="ignore"):
        return np.array([fn(ctypes.c_void_p(base + i * step), ctypes.c_void_p(base + i * step), w, E) for i in range(x.shape[0])], dtype=np.float32)


def quantise(v: np.ndarray, inv: np.ndarray, scale: np.ndarray):
    """(t int32, fp32 root of the measured squared error) of fp32 rows v with per-row inv / scale (fp32 column vectors)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.rint((v * inv).astype(np.float32))
        t = np.where(np.isnan(t), f32(-127.0), t)                     # fminf(fmaxf(NaN, -127), 127)
        t = np.clip(t, -127.0, 127.0).astype(np.float32)
        d = (v - (t * scale).astype(np.float32)).astype(np.float32)
        e2 = (d.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
        root = np.sqrt(e2).astype(np.float32)
    return t.astype(np.int32), root


class Model:
    """The int8 leg's view of one index (raw rows, storage dtype) and one block of raw queries."""

    def __init__(self, space: str, raw_rows: np.ndarray, dtype: str, raw_queries: np.ndarray):
        assert space in ("ip", "l2", "cosine")
        self.space, self.dtype = space, dtype
        if space == "cosine":
            stored = o.normalize_rows(raw_rows) if dtype == "f32" else o.to_storage(o.normalize_rows(raw_rows), dtype)
            self.q = o.normalize_rows(raw_queries)
        else:
            stored = sr.stored(raw_rows, dtype)
            self.q = sr.clean(raw_queries, stored.shape[1])
        self.W = o.widen(stored, dtype)                                # [n, dpad] fp32
        self.n, self.dpad = self.W.shape
        E = o.lib().oracle_elems_per_chunk(o._DT_BY_NAME[dtype])
        # rows
        W8 = pad128(self.W)
        nb = (self.n + 31) // 32
        blk = np.zeros((nb * 32, W8.shape[1]), dtype=np.float32)
        blk[: self.n] = W8
        vmax = np.abs(blk).reshape(nb, -1).max(axis=1)
        with np.errstate(over="ignore", divide="ignore"):
            s_blk = np.where(vmax > 0, (vmax / f32(127.0)).astype(np.float32), f32(1.0)).astype(np.float32)
            inv = (f32(1.0) / s_blk).astype(np.float32)
        self.s_row = np.repeat(s_blk, 32)[: self.n]
        self.tc, root = quantise(W8, np.repeat(inv, 32)[: self.n, None], self.s_row[:, None])
        with np.errstate(over="ignore", invalid="ignore"):
            self.e_r = f32((root * UP + f32(1e-7)).astype(np.float32).max())
        self.rn2 = canon_sq(self.W, E)
        with np.errstate(over="ignore", invalid="ignore"):
            Rrow = (np.sqrt(self.rn2).astype(np.float32) * UP + f32(1e-7)).astype(np.float32)
        self.R = f32(np.inf) if not np.isfinite(Rrow).all() else f32(Rrow.max())
        # queries
        q8 = pad128(self.q)
        qmax = np.abs(q8).max(axis=1)
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            self.s_q = np.where(qmax > 0, (qmax / f32(127.0)).astype(np.float32), f32(0.0)).astype(np.float32)
            qinv = np.where(qmax > 0, (f32(127.0) / qmax).astype(np.float32), f32(0.0)).astype(np.float32)
        self.tq, self.qroot = quantise(q8, qinv[:, None], self.s_q[:, None])
        self.n_q = canon_sq(self.q, 4)

    def slack(self) -> np.ndarray:
        """eps(q), fp32 [B], in prep_queries8_raw_kernel's operations (cosine: prep_queries8_kernel's device-wide bound)"""
        with np.errstate(over="ignore", invalid="ignore"):
            if self.space == "cosine":
                eq = (self.qroot * UP + f32(1e-7)).astype(np.float32)
                return (eq * (f32(1.01) + self.e_r) + f32(1.001) * self.e_r + f32(2e-6)).astype(np.float32)
            m = f32(self.dpad // 64)
            R = self.R
            Q = (np.sqrt(self.n_q).astype(np.float32) * UP + f32(1e-7)).astype(np.float32)
            eq = (self.qroot * UP + U23 * Q + f32(1e-7)).astype(np.float32)
            er = f32(self.e_r * UP + U23 * R)
            a, b = ((Q + eq) * UP).astype(np.float32), f32((R + er) * UP)
            quant = ((eq * b + Q * er * UP) * UP).astype(np.float32)
            if self.space == "l2":
                s = ((a + b) * UP).astype(np.float32)
                rng = (s * s).astype(np.float32)
                eps = ((f32(2.0) * quant + (f32(2.0) * m + f32(18.0)) * U24 * f32(1.001) * rng) * UP + f32(1e-30)).astype(np.float32)
            else:
                rng = (a * b).astype(np.float32)
                eps = ((quant + (m + f32(9.0)) * U24 * f32(1.001) * rng) * UP + f32(1e-30)).astype(np.float32)
            bad = ~((rng >= BAND_LO) & (rng <= BAND_HI)) | ~(eps < np.inf)
            return np.where(bad, f32(np.inf), eps).astype(np.float32)

    def values(self) -> np.ndarray:
        """[B, n] fp32 filter values"""
        acc = self.tq.astype(np.int64) @ self.tc.astype(np.int64).T          # exact
        with np.errstate(over="ignore", invalid="ignore"):
            p = (acc.astype(np.float32) * self.s_row[None, :]).astype(np.float32)
            if self.space != "l2":
                return (p * self.s_q[:, None]).astype(np.float32)
            w = (p.astype(np.float64) * (2.0 * self.s_q.astype(np.float64))[:, None] - self.rn2.astype(np.float64)[None, :]).astype(np.float32)
            return (w - self.n_q[:, None]).astype(np.float32)

    def exact64(self) -> np.ndarray:
        """[B, n] fp64 scores of the stored rows: <q, c>, or -|q - c|^2"""
        Wd, Qd = self.W.astype(np.float64), self.q.astype(np.float64)
        if self.space != "l2":
            return Qd @ Wd.T
        return -np.stack([((Wd - qv[None, :]) ** 2).sum(axis=1) for qv in Qd])

    def ideal_hits(self, k: int) -> np.ndarray:
        """per query: rows whose filter value is within eps(q) of the fp64 k-th best score — what the filter lets through when the
        anchors are the true top-k (the sample can only do worse, and does so alike for every space)"""
        ex, v, eps = self.exact64(), self.values(), self.slack().astype(np.float64)
        kth = np.sort(ex, axis=1)[:, -k]
        return (v.astype(np.float64) >= (kth - eps)[:, None]).sum(axis=1)


def decades(rng, n, d, lo=1e-3, hi=1e3):
    return (rng.standard_normal((n, d)) * np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 1)))).astype(np.float32)


def inputs(kind, N, B, d, dtype="f32", seed=0):
    """(raw rows [N, d], raw queries [B, d]) of one named input of tests/test_space_filter_bound.py and tests/test_gpu_space_filter.py"""
    rng = np.random.default_rng(seed + d)
    raw, q = decades(rng, N, d), decades(rng, B, d)
    if kind == "few_valued":                          # 239 equal entries, the rest zero; rows of three magnitudes
        raw = np.zeros((N, d), dtype=np.float32)
        for i in range(N):
            raw[i, rng.permutation(d)[: min(239, d)]] = np.float32([0.0647, 12.5, 3e-3][i % 3] * (1 if i % 2 else -1))
        q[:4] = raw[:4]
    elif kind == "one_giant_row":
        raw = rng.standard_normal((N, d)).astype(np.float32)
        raw[77] *= np.float32(1e4)
        q = rng.standard_normal((B, d)).astype(np.float32)
        q[1] = raw[77]
    elif kind == "single_large_element":
        raw = rng.standard_normal((N, d)).astype(np.float32)
        raw[np.arange(0, N, 7), rng.integers(0, d, len(range(0, N, 7)))] = np.float32(900.0)
        q = rng.standard_normal((B, d)).astype(np.float32)
        q[np.arange(0, B, 3), rng.integers(0, d, len(range(0, B, 3)))] = np.float32(-2500.0)
    elif kind == "zeros":
        raw[[0, 5, 33, N - 12]] = 0.0
        raw[6, 3] = np.nan                            # (a row with a NaN is the zero row)
        q[[0, 7]] = 0.0
        q[3, 1] = np.inf
    else:
        assert kind == "gaussian_decades"
    if dtype == "f16":                                # fp16 storage holds |x| < 65504
        raw = np.clip(raw, -6e4, 6e4)
    return raw, q


KINDS = ["gaussian_decades", "few_valued", "one_giant_row", "single_large_element", "zeros"]
