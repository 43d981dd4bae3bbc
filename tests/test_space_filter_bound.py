"""The slack of the int8 filter leg of an ip or l2 index held to fp64, on the CPU: for every (query, row) of every
input below, the fp32 filter value as the device computes it (tests/_space_filter_reference.py) lies within eps(q) of the fp64
score of the stored row — <q, c>, or -|q - c|^2.  The bound is the whole soundness argument of the leg (the exact re-score sees
every row whose value is within eps(q) of the anchors' smallest exact score), so it is checked where the unit-norm constants of the
cosine bound would be wrong by orders of magnitude: norms over six decades, one row 10^4 times the rest, single large elements,
few-valued rows, zero vectors; and not vacuously: it must stay a usable number on ordinary data."""

import numpy as np
import pytest

from tests import _space_filter_reference as fr

N, B = 512, 12


@pytest.mark.parametrize("space", ["ip", "l2"])
@pytest.mark.parametrize("d", [200, 768])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", fr.KINDS)
def test_filter_value_within_eps_of_the_fp64_score(space, d, dtype, kind):
    raw, q = fr.inputs(kind, N, B, d, dtype)
    m = fr.Model(space, raw, dtype, q)
    eps = m.slack().astype(np.float64)
    assert not np.isnan(eps).any() and (eps > 0).all()
    err = np.abs(m.values().astype(np.float64) - m.exact64())
    worst = (err / eps[:, None]).max()
    print(space, d, dtype, kind, "largest error / eps(q):", worst, "eps:", eps.min(), "..", eps.max())
    assert (err <= eps[:, None]).all(), (worst, np.argwhere(err > eps[:, None])[:4])
    assert np.isfinite(eps).all(), "finite inputs of this size have a finite bound"


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_the_bound_is_not_vacuous_on_unit_data(space):
    """Unit rows and unit queries: eps_ip is the cosine filter's eps (0.02 at 768 elements) up to the small gamma term, and eps_l2
    exactly twice that for a value that is twice as steep."""
    rng = np.random.default_rng(3)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)  # noqa: E731
    raw, q = unit(rng.standard_normal((N, 768))), unit(rng.standard_normal((B, 768)))
    eps = fr.Model(space, raw, "f32", q).slack()
    cos = fr.Model("cosine", raw, "f32", q).slack()
    scale = 2.0 if space == "l2" else 1.0
    print(space, "eps / (scale * cosine eps):", (eps / (scale * cos)).min(), "..", (eps / (scale * cos)).max())
    assert (eps < 1.02 * scale * cos).all() and (eps > 0.9 * scale * cos).all()


def test_predicted_hit_counts_on_unit_data():
    """The prediction tests/test_gpu_space_filter.py::test_not_vacuous is held against: with ideal anchors (the true top-k) the ip
    and the l2 leg let through as many rows as the cosine int8 filter on the same unit data — far below its factor two."""
    rng = np.random.default_rng(5)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)  # noqa: E731
    raw, q = unit(rng.standard_normal((6144, 768))), unit(rng.standard_normal((64, 768)))
    hits = {s: int(fr.Model(s, raw, "f32", q).ideal_hits(10).sum()) for s in ("cosine", "ip", "l2")}
    print("predicted hits of 64 queries over 6,144 unit rows:", hits)
    assert hits["ip"] < 1.1 * hits["cosine"] and hits["l2"] < 1.1 * hits["cosine"]


def test_a_bound_that_cannot_be_evaluated_is_infinite():
    rng = np.random.default_rng(1)
    raw = rng.standard_normal((64, 200)).astype(np.float32)
    raw[9] *= np.float32(1e19)                        # |c|^2 overflows fp32
    q = rng.standard_normal((4, 200)).astype(np.float32)
    for space in ("ip", "l2"):
        assert np.isposinf(fr.Model(space, raw, "f32", q).slack()).all()
    raw[9] = rng.standard_normal(200).astype(np.float32)
    q[2] *= np.float32(1e19)
    for space in ("ip", "l2"):
        eps = fr.Model(space, raw, "f32", q).slack()
        assert np.isposinf(eps[2]) and np.isfinite(eps[[0, 1, 3]]).all()
