"""Cosine similarity from the RAW inputs in numpy fp64: a reference that owes nothing to the canonical expression.

Every other fp64 check of the suite starts from rows that oracle.normalize_rows has already normalised, and that function restates
the ingest kernel literally: a defect of the canonical normalisation is shared by both sides and bit-for-bit parity cannot see it.
Here the only things taken from the oracle are the two-byte roundings (to_storage / widen: plain format conversions).

The contract
    a vector with a non-finite element, or with no non-zero element, is the zero vector: score 0, distance 1
    any other vector is x / |x|, in fp64 (fp32 inputs: the squares span 1e-90 .. 1e77, their sums stay far inside fp64's range)
    stored rows of a two-byte index are that unit vector rounded to fp32, then to the storage type, then widened
    scores are Q @ C.T in fp64

The tolerance is derived, not measured:   tol(dtype, dpad) = 2e-6 + 2 delta(dpad) + u(dtype)

    2e-6          the project's TOL_F64: what the canonical fp32 dot product of two unit vectors may differ from fp64 by
    delta(dpad)   = ((dpad / 64 + 6) / 2 + 2) * 2^-24 bounds | |stored fp32 vector| - 1 |.  The sum of squares adds positive terms
                  only: 64 chains of dpad / 64 fmas and 6 butterfly levels, so at most dpad / 64 + 6 roundings of 2^-24 relative lie
                  on the way of any term.  The square root halves that relative error and adds one rounding; the division adds
                  another.  Both the query and the row carry it, and the score is bilinear: 2 delta.
    u(dtype)      the storage rounding of the row, as a bound on |row the kernel stores - row of this reference|:
                  f32 0; bf16 2^-8 (half an ulp of an 8-bit significand is 2^-9 relative per element; the kernel rounds a value that
                  is delta away from the one rounded here, which can move an element to the neighbouring bf16 number: 2^-8);
                  f16 2^-11 + sqrt(dpad) * 2^-25 (11-bit significand, and below 2^-14 an absolute half-step of 2^-25 per element).

What is compared
    distances: |(1 - distance) - fp64 score of the returned row| <= tol at every position that holds a row
    ids: only where the reference's own ranking is decided: position j is compared when the fp64 scores at ranks j - 1, j, j + 1
         differ by more than 2 tol (as tests/test_oracle.py does for its fp64 check); the rest is "left out"
    every caller asserts that at most CAP = 10 % of the (query, rank) positions of non-zero queries are left out, so the id
    comparison cannot become vacuous.  A zero query has no ranking in fp64 (every score is 0); its answer is pinned exactly instead:
    rows 0 .. k - 1 at distance 1.0.

Where the cap can hold.  Random background rows of width d score N(0, 1/d) against any unit query; the best of 6,000 reaches about
4 / sqrt(d) and the top ten lie 0.1 / sqrt(d) apart or closer.  Against 2 tol = 6e-6 (f32) that is decided; against 8e-3 (bf16) or
1e-3 (f16) it is not.  Tests on two-byte storage therefore use `crafted_queries`: q = pinv(C_sel).T s gives the chosen rows exactly the
scores s, spaced 2.5 tol apart and starting above the background.  Since sum s_j^2 <= |q|^2 = 1 (Bessel), at most about
1 / (4 / sqrt(d))^2 = d / 16 rows can sit above the background at all: k = 128 at d = 384 cannot be decided by any query, and such a
test asserts the cap over its first ten ranks only (and prints the share over all k).
"""

from __future__ import annotations

import numpy as np

from oracle import knn_oracle as o

TOL_F64 = 2e-6
CAP = 0.10


def delta(dpad: int) -> float:
    return ((dpad / 64 + 6) / 2 + 2) * 2.0**-24


def storage_u(dtype: str, dpad: int) -> float:
    return {"f32": 0.0, "bf16": 2.0**-8, "f16": 2.0**-11 + np.sqrt(dpad) * 2.0**-25}[dtype]


def tol(dtype: str, dpad: int) -> float:
    return TOL_F64 + 2 * delta(dpad) + storage_u(dtype, dpad)


def unit64(x: np.ndarray) -> np.ndarray:
    """fp32 [n, d] -> fp64 [n, pad_dim(d)] unit vectors; zero vectors for rows with a non-finite element or no non-zero one"""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((x.shape[0], o.pad_dim(x.shape[1])), dtype=np.float64)
    x64 = x.astype(np.float64)
    good = np.isfinite(x64).all(axis=1) & (x64 != 0).any(axis=1)
    out[good, : x.shape[1]] = x64[good] / np.sqrt((x64[good] * x64[good]).sum(axis=1, keepdims=True))
    return out


def is_zero_vector(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return ~(np.isfinite(x).all(axis=1) & (x != 0).any(axis=1))


def stored64(raw: np.ndarray, dtype: str) -> np.ndarray:
    u = unit64(raw)
    if dtype == "f32":
        return u
    return o.widen(o.to_storage(u.astype(np.float32), dtype), dtype).astype(np.float64)


def scores64(q_raw: np.ndarray, raw: np.ndarray, dtype: str) -> np.ndarray:
    """[B, n] fp64 cosine of every raw query against every raw row as an index of `dtype` stores it"""
    return unit64(q_raw) @ stored64(raw, dtype).T


def decided(S: np.ndarray, k: int, t: float) -> np.ndarray:
    """(order [B, k] rows by descending fp64 score, ties -> lower row, -1 padded; decided [B, k] bool)"""
    B, n = S.shape
    kk = min(k + 1, n)
    order = np.lexsort((np.broadcast_to(np.arange(n), S.shape), -S), axis=1)[:, :kk]
    s = np.take_along_axis(S, order, axis=1)
    gap = np.full((B, k + 1), np.inf)                       # gap[:, j] = s[j - 1] - s[j]; rank 0 has nobody above, the last row nobody below
    m = min(kk, k + 1)
    gap[:, 1:m] = s[:, : m - 1] - s[:, 1:m]
    dec = (gap[:, :k] > 2 * t) & (gap[:, 1 : k + 1] > 2 * t)
    ids = np.full((B, k), -1, dtype=np.int64)
    ids[:, : min(k, n)] = order[:, : min(k, n)]
    dec[:, min(k, n) :] = False
    return ids, dec


def check(dist: np.ndarray, rows: np.ndarray, q_raw: np.ndarray, S: np.ndarray, t: float, what="", cap_ranks: int | None = None) -> float:
    """One answer (distances [B, k], rows [B, k], -1 padded) against the fp64 scores S [B, n] under the rule above.  Returns the
    left-out share of the positions of non-zero queries (over the first cap_ranks ranks if given), after asserting it <= CAP."""
    dist, rows = np.asarray(dist), np.asarray(rows)
    B, k = rows.shape
    n = S.shape[1]
    zero_q = is_zero_vector(q_raw)
    have = rows >= 0
    assert np.array_equal(have, np.broadcast_to(np.arange(k) < n, (B, k))), (what, "padding")
    assert np.isfinite(dist[have]).all(), (what, "a non-finite distance beside a real row")
    # distances, everywhere
    got = 1.0 - dist.astype(np.float64)
    want = np.take_along_axis(S, np.where(have, rows, 0), axis=1)
    err = np.abs(got - want)[have]
    assert err.size == 0 or err.max() <= t, (what, f"distance off by {err.max():.3e}, tol {t:.3e}")
    # zero queries: pinned exactly
    if zero_q.any():
        assert (dist[zero_q][have[zero_q]] == 1.0).all(), (what, "zero query: distance is not exactly 1")
        assert np.array_equal(rows[zero_q], np.broadcast_to(np.where(np.arange(k) < n, np.arange(k), -1), (int(zero_q.sum()), k))), (what, "zero query: rows")
    # ids where the reference decides
    live = ~zero_q
    if not live.any():
        return 0.0
    ids, dec = decided(S[live], k, t)
    wrong = dec & (rows[live] != ids)
    assert not wrong.any(), (what, f"{int(wrong.sum())} decided positions differ, first {np.argwhere(wrong)[0].tolist()}")
    r = min(k, n) if cap_ranks is None else min(cap_ranks, k, n)
    share = 1.0 - float(dec[:, :r].mean())
    share_all = 1.0 - float(dec[:, : min(k, n)].mean())
    print(f"{what}: left out {share:.1%} of {int(live.sum())} x {r} positions (all {min(k, n)} ranks: {share_all:.1%}), cap {CAP:.0%}; "
          f"worst distance error {err.max() if err.size else 0.0:.3e} of tol {t:.3e}")
    assert share <= CAP, (what, f"left out {share:.1%} > {CAP:.0%}")
    return share


def crafted_queries(raw: np.ndarray, dtype: str, picks: np.ndarray, t: float, floor: float) -> np.ndarray:
    """One fp32 query per row of picks [B, m]: the query in the span of the picked rows (as stored) whose fp64 scores against them
    are proportional to floor + 2.5 t * (m - j), j = 0 .. m - 1: decided by construction once `floor` clears the background."""
    C = stored64(raw, dtype)
    out = np.empty((picks.shape[0], raw.shape[1]), dtype=np.float32)
    for b, sel in enumerate(picks):
        s = floor + 2.5 * t * (len(sel) - np.arange(len(sel)))
        q = np.linalg.pinv(C[sel]) @ s                      # <C[sel][j], q> = s[j]
        nq = np.linalg.norm(q)
        assert nq < 1.0, "the scores asked for cannot be reached by a unit vector"
        out[b] = (q / nq)[: raw.shape[1]].astype(np.float32)
    return out
