"""Corpora that make the k-th place decisive, and their bit-exact reference, for tests/test_gpu_k_boundaries.py (the device side)
and tests/test_k_boundary_premises.py (the conditions under which those tests mean what they say, without a device).

The corpus of one row form (space, n, d, storage dtype)
    ordinary rows   Gaussian (ip / l2: norms scaled by 0.5 .. 1.5)
    planted rows    row(t, s) = s (q + t w) around a query q, w orthogonal to q with |w| = |q|: cosine 1 / sqrt(1 + t^2),
                    squared distance |q|^2 ((s - 1)^2 + s^2 t^2), inner product s |q|^2.  Cosine and l2 order them by t at s = 1,
                    ip by s.
    query PLATEAU   3 distinct best rows, then NPLATEAU byte-identical rows (one raw row stored NPLATEAU times), then the rest.
                    For every k in 4 .. 143 the k-th place falls inside the plateau: the one right answer is the 3 best and the
                    k - 3 LOWEST-SLOT clones.
    query NOTIE     Gaussian, turned away from the clones (which tie under every query) so that they rank last; no tie among its
                    130 best.  The queries from EXTRA on are more of the same.
    query ZERO      all zeros: every score 0 (l2: -|c|^2); cosine and ip answer with the first k live, allowed rows in slot order
    query NEAR      NNEAR rows planted at strictly decreasing closeness, at slots in no order: the rank order is forced
    The 273 planted rows sit at slots drawn from all n without replacement: different waves, workgroups, scan parts, mask words,
    filter tiles and (by the tests' assignment) IVF lists.

The reference scores every (query, row) pair ONCE per form: score_word[q, r], the high word of the packed key of DESIGN.md §2
(cosine and ip: oracle.knn_oracle.search_keys over blocks of 64 stored rows; l2: tests/_space_reference.l2_matrix).  Every k and
every restriction (scope, mask, tombstones, probed lists, a sub-index of some of the rows) is a selection from that table:
key = score_word << 32 | (0xFFFFFFFF - row_base - slot), the k largest among the member rows, descending, 0 padded.  No tolerance."""

from __future__ import annotations

import numpy as np

from oracle import knn_oracle as o
from tests import _space_reference as sr

KS = (1, 2, 16, 17, 63, 64, 65, 127, 128)
KMAX = 128
NBEST, NPLATEAU, NNEAR = 3, 140, 130
PLATEAU, NOTIE, ZERO, NEAR, EXTRA = 0, 1, 2, 3, 4
NQ = 8
LOW = np.uint64(0xFFFFFFFF)

# closeness of the planted rows: t (cosine, l2; s = 1) and s (ip; t = T_CLONE)
T_BEST, T_CLONE = (0.05, 0.10, 0.15), 0.30
S_BEST, S_CLONE = (2.6, 2.5, 2.4), 2.0


def t_near(i):
    return 0.05 + 0.006 * i


def s_near(i):
    return 3.0 - 0.008 * i


def _planted(q, w, t, s):
    return (s * (q.astype(np.float64) + t * w)).astype(np.float32)


def _orthogonal(rng, q):
    q64 = q.astype(np.float64)
    w = rng.standard_normal(q.shape[0])
    w -= q64 * (w @ q64) / (q64 @ q64)
    return w * np.linalg.norm(q64) / np.linalg.norm(w)


class Corpus:
    """raw rows and queries of one form, the planted slots, and score_word [NQ, n]"""

    # Among 33,301 fp32 cosines two of a Gaussian query's 130 best can share a word by chance: such a form takes another seed
    # (check_premises says when one is needed)
    SEEDS = {("cosine", 33_301, 384, "f32"): 1}

    def __init__(self, space: str, n: int, d: int, dtype: str, seed: int | None = None):
        assert n >= NBEST + NPLATEAU + NNEAR + 64
        seed = self.SEEDS.get((space, n, d, dtype), 0) if seed is None else seed
        self.space, self.n, self.d, self.dtype = space, n, d, dtype
        rng = np.random.default_rng(9000 + 7 * d + n + seed)
        raw = rng.standard_normal((n, d)).astype(np.float32)
        if space != "cosine":
            raw *= rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
        q = rng.standard_normal((NQ, d)).astype(np.float32)
        q[ZERO] = 0.0
        slots = rng.permutation(rng.choice(n, size=NBEST + NPLATEAU + NNEAR, replace=False))
        self.best = slots[:NBEST].astype(np.int64)                                   # rank order
        self.plateau = np.sort(slots[NBEST : NBEST + NPLATEAU]).astype(np.int64)     # slot order = rank order
        self.near = slots[NBEST + NPLATEAU :].astype(np.int64)                       # rank order, slots in no order
        ip = space == "ip"
        w = _orthogonal(rng, q[PLATEAU])
        for j in range(NBEST):
            raw[self.best[j]] = _planted(q[PLATEAU], w, T_CLONE if ip else T_BEST[j], S_BEST[j] if ip else 1.0)
        raw[self.plateau] = _planted(q[PLATEAU], w, T_CLONE, S_CLONE if ip else 1.0)
        # the clones tie under EVERY query: the no-tie queries point away from them (cosine -0.5), so they rank at the bottom there
        clone = raw[self.plateau[0]].astype(np.float64)
        for j in [NOTIE, *range(EXTRA, NQ)]:
            q64 = q[j].astype(np.float64)
            q64 -= (q64 @ clone / (clone @ clone) + 0.5 * np.linalg.norm(q64) / np.linalg.norm(clone)) * clone
            q[j] = q64.astype(np.float32)
        w = _orthogonal(rng, q[NEAR])
        for i in range(NNEAR):
            raw[self.near[i]] = _planted(q[NEAR], w, T_CLONE if ip else t_near(i), s_near(i) if ip else 1.0)
        self.raw, self.queries = raw, q
        if space == "cosine":
            self.stored, self.qprep = o.to_storage(o.normalize_rows(raw), dtype), o.normalize_rows(q)
        else:
            self.stored = sr.stored(raw, dtype)
            self.qprep = sr.clean(q, self.stored.shape[1])
        self.score_word = score_words(space, self.stored, dtype, self.qprep)
        self.planted = np.sort(slots).astype(np.int64)

    def batch(self, B: int, half_plateau: bool = False) -> np.ndarray:
        """query numbers of a batch of B: PLATEAU, NOTIE, ZERO, NEAR, the extra ones, and round again; half_plateau: the upper half
        of the batch is the plateau query"""
        qidx = np.arange(B) % NQ
        if half_plateau:
            qidx[B // 2 :] = PLATEAU
        return qidx


def score_words(space, stored, dtype, qprep) -> np.ndarray:
    """uint32 [B, n]: the high word of each pair's packed key"""
    n = stored.shape[0]
    if space == "l2":
        return sr.ord_f32(np.float32(0.0) - sr.l2_matrix(stored, dtype, qprep))
    out = np.zeros((qprep.shape[0], n), dtype=np.uint32)
    for a in range(0, n, 64):
        blk = np.ascontiguousarray(stored[a : a + 64])
        keys = o.search_keys(blk, dtype, qprep, blk.shape[0], a)
        at = (LOW - (keys & LOW)).astype(np.int64)
        assert (keys != 0).all()
        np.put_along_axis(out, at, (keys >> np.uint64(32)).astype(np.uint32), axis=1)
    return out


def top_keys(score_word, member, k=KMAX, row_base=0, slots=None) -> np.ndarray:
    """u64 [B, k]: the k largest keys among the member rows (bool [n] or [B, n]), descending, 0 padded.  slots: the slot each column
    of score_word has in the searched index (default: its own number)."""
    score_word = np.atleast_2d(score_word)
    B, n = score_word.shape
    slots = np.arange(n, dtype=np.int64) if slots is None else np.asarray(slots, dtype=np.int64)
    keys = (score_word.astype(np.uint64) << np.uint64(32)) | (np.int64(0xFFFFFFFF) - row_base - slots).astype(np.uint64)[None, :]
    keys = np.where(np.broadcast_to(np.asarray(member, dtype=bool), (B, n)), keys, np.uint64(0))
    out = np.zeros((B, k), dtype=np.uint64)
    kk = min(k, n)
    out[:, :kk] = np.sort(keys, axis=1)[:, ::-1][:, :kk]
    return out


def unpack(space, keys, row_base=0):
    """(distances fp32, rows int64) of packed keys: what the search writes beside them"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if space == "cosine":
        dist, rows = o.unpack_keys(keys)
        return dist, np.where(rows >= 0, rows - row_base, -1)
    rows = sr.key_rows(keys, row_base)
    return sr.distances(space, sr.key_scores(keys), rows >= 0), rows


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def words_of(mask: np.ndarray, garbage_above: bool = True) -> np.ndarray:
    """packed uint32 mask words; the bits at or above the count are set, and to be ignored"""
    n = mask.shape[0]
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    words = words.view("<u4").copy()
    if garbage_above and n % 32:
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)
    return words


# ---- the premises ----------------------------------------------------------------------------------------------------------------
def check_premises(c: Corpus) -> None:
    """What makes the cut decisive: the plateau is ONE score word, the 3 best lie strictly above it in their order, every other row
    strictly below; the near-duplicates lie strictly in their planted order above every other row; the no-tie queries have no tie
    among their KMAX + 2 best; the zero query scores every row 0 (l2: by norm)."""
    w = c.score_word
    p = w[PLATEAU]
    assert len(set(map(bytes, c.stored[c.plateau]))) == 1, "the clones are not byte-identical as stored"
    level = p[c.plateau[0]]
    assert (p[c.plateau] == level).all(), "the plateau has more than one score word"
    b = p[c.best].astype(np.int64)
    assert (np.diff(b) < 0).all() and b[-1] > level, "the 3 best are not strictly ordered above the plateau"
    rest = np.ones(c.n, dtype=bool)
    rest[c.best] = rest[c.plateau] = False
    assert (p[rest] < level).all(), "a row outside the plateau reaches it"
    nd = w[NEAR][c.near].astype(np.int64)
    assert (np.diff(nd) < 0).all(), "the planted order is not strict"
    rest = np.ones(c.n, dtype=bool)
    rest[c.near] = False
    assert (w[NEAR][rest] < nd[-1]).all(), "an ordinary row reaches the near-duplicates"
    for q in [NOTIE, *range(EXTRA, NQ)]:
        top = np.sort(w[q])[::-1][: KMAX + 2].astype(np.int64)
        assert (np.diff(top) < 0).all(), ("a tie among the best of a no-tie query", q)
    if c.space != "l2":
        assert (w[ZERO] == w[ZERO][0]).all() and sr.unord_f32(w[ZERO][:1])[0] == 0.0


def plateau_answer(c: Corpus, k: int) -> np.ndarray:
    """the rows of the plateau query's answer at k, stated directly: the 3 best, then the lowest-slot clones"""
    return np.concatenate([c.best, c.plateau])[:k]
