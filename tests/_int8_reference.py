"""numpy restatement of the int8 shadow (shadow8_from_rows_kernel, prep_queries8_kernel and the DUMP pass behind
codd_knn_approx_scores): the same fp32 operations, so scores compare bit for bit."""

from __future__ import annotations

import numpy as np


def quantise_like_the_kernels(x, is_query):
    """fp32 arithmetic of shadow8_from_rows_kernel / prep_queries8_kernel.  Stored rows share ONE scale per 32-row block (the
    block's largest magnitude / 127); a query has its own."""
    x = x.astype(np.float32)
    vmax = np.abs(x).max(axis=1).astype(np.float32)
    if not is_query:
        pad = (-len(vmax)) % 32
        vmax = np.repeat(np.concatenate([vmax, np.zeros(pad, np.float32)]).reshape(-1, 32).max(axis=1), 32)[: x.shape[0]]
    safe = np.where(vmax > 0, vmax, np.float32(1.0)).astype(np.float32)
    if is_query:
        scale = np.where(vmax > 0, vmax / np.float32(127.0), np.float32(0.0)).astype(np.float32)
        inv = np.where(vmax > 0, np.float32(127.0) / safe, np.float32(0.0)).astype(np.float32)
    else:
        scale = np.where(vmax > 0, vmax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
        inv = (np.float32(1.0) / scale).astype(np.float32)
    q8 = np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -127, 127).astype(np.int32)
    return q8, scale


def int8_scores(rows_f32, qn):
    """[B, n] fp32: what approx_scores returns for the widened stored rows and the normalised queries qn on the int8 shadow"""
    c8, cs = quantise_like_the_kernels(rows_f32, False)
    q8, qs = quantise_like_the_kernels(qn, True)
    acc = (q8.astype(np.float64) @ c8.astype(np.float64).T).astype(np.float32)  # integers, |acc| < 2^24: exact in fp64 and in fp32
    return ((acc * cs[None, :]).astype(np.float32) * qs[:, None]).astype(np.float32)


def row_error_norms(rows_f32):
    """[n] fp64 quantisation error norms |c - c~| of the stored rows (bmeta's second field is the largest of a block, inflated by 1e-4)"""
    c8, cs = quantise_like_the_kernels(rows_f32, False)
    return np.linalg.norm(rows_f32.astype(np.float64) - c8.astype(np.float64) * cs[:, None].astype(np.float64), axis=1)


def int8_parts(rows_f32, q):
    """(acc int64 [B, n], row scales fp32 [n], query scales fp32 [B]) of widened stored rows and prepared queries: the exact integer
    accumulators of the int8 GEMM and the two scales its scores are made of.  The integer products are summed in fp32 where every
    partial sum stays below 2^24 (rows of up to 1,040 elements: 127^2 d), else in fp64: exact either way."""
    c8, cs = quantise_like_the_kernels(rows_f32, False)
    q8, qs = quantise_like_the_kernels(q, True)
    wide = np.float32 if 127 * 127 * rows_f32.shape[1] < 2**24 else np.float64
    acc = np.rint(q8.astype(wide) @ c8.astype(wide).T).astype(np.int64)
    return acc, cs, qs


def scores_from_parts(acc, cs, qs):
    """fp32 [B, n]: (p, s~) with p = fp32(acc * s_row), what the kernels' tests run on, and s~ = fp32(p * s_q), what a key carries
    (cosine and ip)"""
    p = (acc.astype(np.float32) * cs[None, :]).astype(np.float32)
    return p, (p * qs[:, None]).astype(np.float32)


def sqd_from_parts(acc, cs, qs, rn2, nq2):
    """fp32 [B, n]: (w, v) of an l2 index's leg: w = fma(fp32(acc * s_row), 2 s_q, -|c|^2), what sqd_filter_kernel
    tests, and v = fp32(w - |q|^2), what a key carries.  rn2 / nq2: the canonical sums of squares of the stored rows and of the
    cleaned queries.  The fma is one rounding of an fp64 expression whose product is exact (two fp32 factors)."""
    p = (acc.astype(np.float32) * cs[None, :]).astype(np.float32)
    s2 = (np.float32(2.0) * qs).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = (p.astype(np.float64) * s2.astype(np.float64)[:, None] - rn2.astype(np.float64)[None, :]).astype(np.float32)
        v = (w - nq2.astype(np.float32)[:, None]).astype(np.float32)
    return w, v
