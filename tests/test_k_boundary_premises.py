"""The conditions under which tests/test_gpu_k_boundaries.py means what it says, checked on the CPU reference alone: per row form the
plateau is one score word with the 3 best strictly above it and everything else strictly below, the planted near-duplicate order is
strict, and the reference's selection returns the lowest-slot clones.  If a storage dtype's rounding breaks strictness the planted
spacing (tests/_k_boundary_cases.py) changes, not these assertions."""

import numpy as np
import pytest

from tests import _k_boundary_cases as kb

# every (space, d, dtype) the device tests build, at the smallest row count they use it with
FORMS = [(space, d, dtype) for d, dtype in ((64, "f32"), (384, "f32"), (768, "f32"), (1536, "f32"), (1024, "f16"), (2048, "f16"), (3072, "f16"))
         for space in ("cosine", "l2")] + [("ip", 64, "f32"), ("ip", 384, "f32"), ("ip", 768, "f32"), ("ip", 1024, "f16"), ("ip", 1536, "f32")]


@pytest.mark.parametrize("space,d,dtype", FORMS, ids=[f"{s}-{d}-{t}" for s, d, t in FORMS])
def test_the_cut_is_decisive(space, d, dtype):
    c = kb.Corpus(space, 1_501, d, dtype)
    kb.check_premises(c)
    everyone = np.ones(c.n, dtype=bool)
    top = kb.top_keys(c.score_word, everyone)
    for k in kb.KS:
        dist, rows = kb.unpack(space, top[:, :k])
        assert np.array_equal(rows[kb.PLATEAU], kb.plateau_answer(c, k)), k
        assert np.array_equal(rows[kb.NEAR], c.near[:k]), k
        if space != "l2":
            assert np.array_equal(rows[kb.ZERO], np.arange(k)), k
        assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
    # the plateau's distance is one value, and the cut between k = 64 and 65 moves one clone in
    dist, rows = kb.unpack(space, top[kb.PLATEAU : kb.PLATEAU + 1])
    assert len(set(kb.bits(dist[0, kb.NBEST :]).tolist())) == 1
    assert rows[0, 63] == c.plateau[60] and rows[0, 64] == c.plateau[61] and rows[0, 127] == c.plateau[124]


def test_selections_restrict_pad_and_renumber():
    c = kb.Corpus("cosine", 1_501, 64, "f32")
    # a mask that allows the plateau's upper half only: the lowest allowed clone is not the lowest clone
    mask = np.ones(c.n, dtype=bool)
    mask[c.plateau[:70]] = False
    rows = kb.unpack("cosine", kb.top_keys(c.score_word[kb.PLATEAU], mask, 65))[1][0]
    assert np.array_equal(rows, np.concatenate([c.best, c.plateau[70:132]]))
    # fewer member rows than k: padding (row -1, distance +inf, key 0)
    few = np.zeros(c.n, dtype=bool)
    few[c.planted[:63]] = True
    keys = kb.top_keys(c.score_word, few, 64, row_base=1_000)
    dist, rows = kb.unpack("cosine", keys, row_base=1_000)
    assert (keys[:, 63] == 0).all() and (keys[:, 62] != 0).all() and (rows[:, 63] == -1).all() and np.isinf(dist[:, 63]).all()
    assert set(rows[0, :63].tolist()) == set(c.planted[:63].tolist())
    # a sub-index of some of the rows, renumbered in slot order
    sub = c.planted[:65]
    keys = kb.top_keys(c.score_word[:, sub], np.ones(65, dtype=bool), 66, slots=np.arange(65))
    rows = kb.unpack("cosine", keys)[1]
    assert (np.sort(rows[:, :65], axis=1) == np.arange(65)).all() and (rows[:, 65] == -1).all()
    # a batch repeats the queries in a fixed order
    assert c.batch(9).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0] and (c.batch(256, half_plateau=True)[128:] == kb.PLATEAU).all()
