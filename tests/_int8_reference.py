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
