"""Self-check of tests/_space_reference.py against fp64 on the stored rows: the same arithmetic, wider.

Tolerances, from the roundings on the path (u = 2^-24, L = dpad / 64 chain steps per lane, 6 butterfly levels):
    l2   every term t^2 is non-negative, so errors are relative: one rounding of the subtraction (squared: 2u), one per fma on the
         way of a term (at most L), one per butterfly level (6): relative error <= (L + 8) u.
    ip   terms cancel, so the error is absolute against sum |q_i c_i| <= |q| |c|: (L + 6) u |q| |c|, plus one fp32 rounding of
         1 - s.
Ids are compared where neighbouring fp64 values differ by more than twice that; the share left out is capped at CAP = 10 %."""

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests import _space_reference as sr
from tests._cosine_reference import CAP

U = 2.0**-24
CASES = [(200, 6000, "f32"), (70, 3000, "f16"), (1536, 1500, "bf16")]
K = 10


def inputs(d, n, B=6, seed=5):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = (1.3 * rng.standard_normal((B, d))).astype(np.float32)
    return raw, q


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("d,n,dtype", CASES)
def test_the_reference_agrees_with_fp64_on_the_stored_rows(space, d, n, dtype):
    raw, q = inputs(d, n)
    ref = sr.Reference(space, raw, dtype, q)
    W = o.widen(ref.rows, dtype)
    dpad = W.shape[1]
    _, dist, rows = ref.topk(q.shape[0], K)
    D64 = sr.brute64(space, W, ref.q)
    want = np.take_along_axis(D64, rows, axis=1)
    if space == "l2":
        tol = (dpad / 64 + 8) * U * D64
    else:
        norms = np.linalg.norm(ref.q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(W.astype(np.float64), axis=1)[None, :]
        tol = (dpad / 64 + 6) * U * norms + U * np.maximum(np.abs(D64), 1.0)
    tol_hit = np.take_along_axis(tol, rows, axis=1)
    err = np.abs(dist.astype(np.float64) - want)
    print(f"{space} {dtype} d={d} n={n}: worst error / tolerance {float((err / tol_hit).max()):.3f}")
    assert (err <= tol_hit).all()
    # ids where fp64 decides: rank j is compared when its fp64 neighbours lie more than twice the tolerance away
    order = np.lexsort((np.broadcast_to(np.arange(n), D64.shape), D64), axis=1)[:, : K + 1]
    s = np.take_along_axis(D64, order, axis=1)
    t = np.take_along_axis(tol, order, axis=1)
    gap_ok = (s[:, 1:] - s[:, :-1]) > 2 * np.maximum(t[:, 1:], t[:, :-1])          # [B, K]: between ranks j and j + 1
    decided = gap_ok.copy()
    decided[:, 1:] &= gap_ok[:, :-1]
    assert np.array_equal(rows[decided], order[:, :K][decided])
    share = 1.0 - float(decided.mean())
    print(f"{space} {dtype} d={d} n={n}: left out {share:.1%}, cap {CAP:.0%}")
    assert share <= CAP
    assert np.array_equal(rows, order[:, :K]), "the reference's ids equal fp64's everywhere for these inputs"


def test_key_packing_round_trips_and_orders_like_the_scores():
    s = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32)
    hi = sr.ord_f32(s)
    assert (np.diff(hi.astype(np.int64)) >= 0).all() and np.array_equal(sr.unord_f32(hi).view(np.uint32), s.view(np.uint32))
    keys = sr.make_keys(s, np.arange(7), row_base=0xFFFFFFF6)
    assert np.array_equal(sr.key_rows(keys, 0xFFFFFFF6), np.arange(7)) and keys[-1] & np.uint64(0xFFFFFFFF) == 3
    assert sr.ord_f32(np.array([np.nan], dtype=np.float32))[0] == sr.ord_f32(np.array([-np.inf], dtype=np.float32))[0]
    assert sr.make_keys(s[:1], np.array([-1]))[0] == 0


def test_non_finite_and_zero_vectors_are_the_zero_vector():
    x = np.ones((5, 3), dtype=np.float32)
    x[1, 0], x[2, 2], x[3] = np.nan, -np.inf, 0.0
    x[4] = [-0.0, 0.0, -0.0]
    c = sr.clean(x)
    assert c.shape == (5, 64) and np.array_equal(c[0, :3], [1, 1, 1]) and not c[1:].any() and not np.signbit(c[4]).any()
