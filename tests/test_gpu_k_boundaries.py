"""k at the list-slot boundaries on every search route: KS = 1, 2, 16, 17, 63, 64, 65, 127, 128.

WaveTopK keeps rank r in slot r / 64 of lane r % 64, dispatch.h instantiates every exact-score kernel with one list slot for k <= 64
and with two above, every partial buffer's stride is k, and the routing itself reads k (sample floor max(64, 4k), the filter leg for
ntiles >= 2k only, the fused finalize and the one-launch small batch for k <= 64 only, the wide 2-byte l2 scan's group of 4 or 2).
The corpora of tests/_k_boundary_cases.py put a decisive row on the cut: for 4 <= k <= 143 the plateau query's k-th place lies inside
140 byte-identical rows, so a wrong threshold lane, a lost carry or a stale rank changes WHICH clone comes back.

Every case asserts the route it names ran (stats, last_pass), then compares packed keys, distance bits and rows with the selection
from the form's score table — no tolerance — and, as a cross-check only, with the first k entries of the route's own answer at 128."""

import functools

import numpy as np
import pytest

from codd_query_engine_amd import native
from tests import _filter_stage_reference as fs
from tests import _k_boundary_cases as kb

pytestmark = pytest.mark.gpu
KS = kb.KS
ROW_BASE = 1_000_000
EINVAL = "-22"
SPACES3 = ("cosine", "l2", "ip")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex, ivf


@functools.lru_cache(maxsize=None)
def corpus(space, n, d, dtype):
    c = kb.Corpus(space, n, d, dtype)
    kb.check_premises(c)
    return c


@functools.lru_cache(maxsize=None)
def top_all(space, n, d, dtype):
    c = corpus(space, n, d, dtype)
    return kb.top_keys(c.score_word, np.ones(c.n, dtype=bool))


def open_index(Index, c, options=None, rows=None):
    ix = Index(c.d, dtype=c.dtype, space=c.space)
    for key, value in (options or {}).items():
        ix.set_option(key, value)
    raw = c.raw if rows is None else c.raw[rows]
    if raw.shape[0]:
        ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw, normalize=c.space == "cosine")
    return ix


def keys_of(t):
    return t.cpu().numpy().view(np.uint64)


def based(keys, row_base):
    """the keys of the same rows under a row base"""
    return np.where(keys != 0, keys - np.uint64(row_base), np.uint64(0))


def same_keys(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "queries", bad[:8], "first difference at rank", int(np.flatnonzero(got[bad[0]] != want[bad[0]])[0]),
                           kb.unpack("cosine", got[bad[:1]])[1][0][-4:], kb.unpack("cosine", want[bad[:1]])[1][0][-4:])


def same_answer(space, got, want_keys, what):
    """(dist, rows) as a search wrote them against the reference keys unpacked: rows, then distance bits"""
    dist, rows = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    d_ref, r_ref = kb.unpack(space, want_keys)
    bad = np.flatnonzero((rows != r_ref).any(axis=1))
    assert bad.size == 0, (what, "rows of queries", bad[:8], rows[bad[0]][-4:], r_ref[bad[0]][-4:])
    assert np.array_equal(kb.bits(dist), kb.bits(d_ref)), (what, "distance bits")


def ks_desc(ks=KS):
    return sorted(ks, reverse=True)


# ---- 1. the exact scan -----------------------------------------------------------------------------------------------------------
SCAN_FORMS = [(64, "f32"), (768, "f32"), (2048, "f16"), (1536, "f32"), (3072, "f16")]
SCAN_CASES = [(s, d, t) for d, t in SCAN_FORMS for s in ("cosine", "l2")] + [("ip", 768, "f32")]
WIDE = {(1536, "f32"), (3072, "f16")}


def scan_group(space, d, dtype, B, k):
    """queries per pass over the rows, as DESIGN.md §6 and §20 state it: 1, 4 or 8 by the batch; wide 2-byte rows at most 4, and 2
    under l2 with two list slots (k > 64)"""
    nb = 1 if B == 1 else (4 if B <= 4 else 8)
    if (d, dtype) in WIDE and dtype != "f32" and nb >= 4:
        return 2 if (space == "l2" and k > 64) else 4
    return nb


@pytest.mark.parametrize("space,d,dtype", SCAN_CASES, ids=[f"{s}-{d}-{t}" for s, d, t in SCAN_CASES])
def test_exact_scan(env, space, d, dtype):
    _, Index, _ = env
    c = corpus(space, 1_501, d, dtype)
    top = top_all(space, 1_501, d, dtype)
    ix = open_index(Index, c, {"filter": 0})
    assert np.array_equal(ix.read_rows(), c.stored), "ingest differs from the reference"
    for B in (1, 4, 9):
        qidx = c.batch(B)
        q = c.queries[qidx]
        at128 = None
        for k in ks_desc():
            before = ix.stat("scan_launches")
            want = top[qidx][:, :k]
            same_answer(space, ix.search(q, k), want, (space, d, dtype, B, k))
            assert ix.stat("last_scan_group") == scan_group(space, d, dtype, B, k), (B, k)
            got = keys_of(ix.search_keys(q, k, ROW_BASE))
            same_keys(got, based(want, ROW_BASE), (space, d, dtype, B, k, "keys"))
            assert ix.stat("scan_launches") == before + 2 and ix.stat("filter_passes") == 0
            at128 = got if k == 128 else at128
            assert np.array_equal(got, at128[:, :k]), ("not a prefix of the answer at 128", B, k)
            if k >= 4:
                assert np.array_equal(kb.unpack(space, got[:1], ROW_BASE)[1][0], kb.plateau_answer(c, k))
    if (d, dtype) == (3072, "f16") and space == "l2":
        ix.search(c.queries[c.batch(4)], 64)
        g64 = ix.stat("last_scan_group")
        ix.search(c.queries[c.batch(4)], 65)
        assert (g64, ix.stat("last_scan_group")) == (4, 2)
    ix.close()


COUNT_CASES = [(s, d, t) for d, t in ((768, "f32"), (3072, "f16")) for s in ("cosine", "l2")]


@pytest.mark.parametrize("space,d,dtype", COUNT_CASES, ids=[f"{s}-{d}-{t}" for s, d, t in COUNT_CASES])
def test_exact_scan_of_an_index_of_k_rows_give_or_take_one(env, space, d, dtype):
    """One index grown row by row out of the planted rows (clones, near-duplicates, the 3 best); at every count m it is searched with
    every k of KS within one of m: m = k - 1 pads one place, m = k fills the last lane, m = k + 1 drops exactly one row."""
    _, Index, _ = env
    c = corpus(space, 1_501, d, dtype)
    sub = c.planted[: kb.KMAX + 1]
    ix = open_index(Index, c, {"filter": 0}, rows=sub[:0])
    qidx = c.batch(9)
    q = c.queries[qidx]
    have = 0
    for m in sorted({k + e for k in KS for e in (-1, 0, 1)}):
        if m > have:
            ix.upsert(np.arange(have, m, dtype=np.int64), c.raw[sub[have:m]], normalize=space == "cosine")
            have = m
        assert ix.count() == m
        for k in [k for k in KS if abs(k - m) <= 1]:
            want = kb.top_keys(c.score_word[:, sub[:m]], np.ones(m, dtype=bool), k, slots=np.arange(m))[qidx]
            same_answer(space, ix.search(q, k), want, (space, d, dtype, "count", m, k))
            same_keys(keys_of(ix.search_keys(q, k, ROW_BASE)), based(want, ROW_BASE), (space, d, dtype, "count keys", m, k))
            assert ((want != 0).sum(axis=1) == min(m, k)).all()
    ix.close()


# ---- 2. scoped search ------------------------------------------------------------------------------------------------------------
EDGE_KS = (63, 64, 65, 127, 128)
EDGE_COUNTS = sorted({k + e for k in EDGE_KS for e in (-1, 0, 1)})         # scope m holds exactly m rows
PLATEAU_SCOPE, UNKNOWN_SCOPE = 1_000, 77_777
SCOPED_CASES = [(s, d, t) for d, t in ((384, "f32"), (2048, "f16")) for s in ("cosine", "l2")]


def scope_labels(c):
    """scope m (m in EDGE_COUNTS): 2 clones, 10 near-duplicates and m - 12 ordinary rows; PLATEAU_SCOPE: 120 clones, one of the 3 best
    and 200 ordinary rows; every other row: scope 0 (none)"""
    rng = np.random.default_rng(c.n + c.d)
    labels = np.zeros(c.n, dtype=np.uint32)
    ordinary = np.ones(c.n, dtype=bool)
    ordinary[c.planted] = False
    free = rng.permutation(np.flatnonzero(ordinary))
    spare = np.concatenate([c.plateau[:10], c.plateau[130:]])
    at = 0
    for i, m in enumerate(EDGE_COUNTS):
        labels[spare[2 * i : 2 * i + 2]] = m
        labels[c.near[10 * i : 10 * i + 10]] = m
        labels[free[at : at + m - 12]] = m
        at += m - 12
    labels[c.plateau[10:130]] = PLATEAU_SCOPE
    labels[c.best[1]] = PLATEAU_SCOPE
    labels[free[at : at + 200]] = PLATEAU_SCOPE
    assert all(int((labels == m).sum()) == m for m in EDGE_COUNTS)
    return labels


def scoped_want(c, labels, qidx, scopes, k):
    member = np.stack([np.ones(c.n, dtype=bool) if s == 0 else labels == s for s in scopes.tolist()])
    return kb.top_keys(c.score_word[qidx], member, k)


@pytest.mark.parametrize("space,d,dtype", SCOPED_CASES, ids=[f"{s}-{d}-{t}" for s, d, t in SCOPED_CASES])
def test_scoped_search(env, space, d, dtype):
    _, Index, _ = env
    c = corpus(space, 6_001, d, dtype)
    labels = scope_labels(c)
    ix = open_index(Index, c)
    ix.set_scopes(np.arange(c.n, dtype=np.int64), labels)
    searches = 0

    def run(qidx, scopes, k):
        nonlocal searches
        want = scoped_want(c, labels, qidx, scopes, k)
        same_answer(space, ix.search_scoped(c.queries[qidx], scopes, k), want, (space, d, dtype, "scoped", scopes[:4], k))
        got = keys_of(ix.search_keys_scoped(c.queries[qidx], scopes, k, ROW_BASE))
        same_keys(got, based(want, ROW_BASE), (space, d, dtype, "scoped keys", scopes[:4], k))
        searches += 2
        assert ix.stat("scoped_searches") == searches, "the scoped entry point did not count the search"
        return want

    # one query (one work item, the list cut into parts): every scope that ends at the padding rule, with the k around its count
    for m in EDGE_COUNTS:
        for k in [k for k in EDGE_KS if abs(k - m) <= 1]:
            for qn in (kb.PLATEAU, kb.NEAR):
                want = run(np.array([qn]), np.array([m], dtype=np.uint32), k)
                assert int((want != 0).sum()) == min(m, k)
    for s in (PLATEAU_SCOPE, 0, UNKNOWN_SCOPE):
        for k in ks_desc():
            want = run(np.array([kb.PLATEAU]), np.array([s], dtype=np.uint32), k)
            rows = kb.unpack(space, want)[1][0]
            if s == PLATEAU_SCOPE:      # one best row, then the scope's 120 clones, lowest slots first
                assert np.array_equal(rows[:121], np.concatenate([c.best[1:2], c.plateau[10:130]])[:k])
            elif s == 0:
                assert np.array_equal(rows, kb.plateau_answer(c, k))
            else:
                assert (want == 0).all()
    # 40 queries over 13 scopes: three or four queries per scope (groups of scope_nb queries and a remainder), scope 0's list in parts
    cycle = np.array(EDGE_COUNTS + [PLATEAU_SCOPE, 0, UNKNOWN_SCOPE, PLATEAU_SCOPE], dtype=np.uint32)
    scopes = np.resize(cycle, 40)
    qidx = (np.arange(40) // len(cycle) + np.arange(40)) % kb.NQ
    at128 = None
    for k in ks_desc():
        want = run(qidx, scopes, k)
        at128 = want if k == 128 else at128
        assert np.array_equal(want, at128[:, :k])
    assert ix.stat("scope_builds") == 1 and ix.stat("filter_passes") == 0
    ix.close()


# ---- 3. masked search ------------------------------------------------------------------------------------------------------------
N_MASK = 7_013                                                               # 219 * 32 + 5: the last mask word is partial
LIST, DENSE = 1, 2
MASKED_CASES = [(s, d, t) for d, t in ((768, "f32"), (2048, "f16")) for s in ("cosine", "l2")]


def dead_rows(c):
    dead = np.zeros(c.n, dtype=bool)
    dead[np.random.default_rng(c.n).choice(c.n, size=c.n // 8, replace=False)] = True
    dead[c.plateau[0]] = True                                                # the lowest clone
    dead[c.plateau[1]] = False
    dead[c.n - 1] = True
    return dead


def visible_order(c):
    """a fixed order of the rows whose every prefix mixes clones, near-duplicates, best and ordinary rows"""
    rng = np.random.default_rng(c.d)
    ordinary = np.ones(c.n, dtype=bool)
    ordinary[c.planted] = False
    head = rng.permutation(np.concatenate([c.planted[::2], np.flatnonzero(ordinary)[: len(c.planted[::2])]]))
    return head


@pytest.mark.parametrize("route", [LIST, DENSE], ids=["list", "dense"])
@pytest.mark.parametrize("space,d,dtype", MASKED_CASES, ids=[f"{s}-{d}-{t}" for s, d, t in MASKED_CASES])
def test_masked_search(env, space, d, dtype, route):
    torch, Index, _ = env
    c = corpus(space, N_MASK, d, dtype)
    order = visible_order(c)
    upper = np.ones(c.n, dtype=bool)
    upper[c.plateau[:70]] = False                                            # the lowest allowed clone is not the lowest clone
    half = np.random.default_rng(17).random(c.n) < 0.5
    qidx = c.batch(9)
    q = c.queries[qidx]
    for dead in (None, dead_rows(c)):
        ix = open_index(Index, c, {"mask_route": route, "filter": 0})
        live = np.ones(c.n, dtype=bool)
        if dead is not None:
            ix.delete(np.flatnonzero(dead))
            live = ~dead

        def run(mask, k, what):
            visible = mask & live
            want = kb.top_keys(c.score_word, visible, k)[qidx]
            words = kb.words_of(mask)
            before = {key: ix.stat(key) for key in ("masked_searches", "mask_list_searches", "mask_dense_searches", "masked_dev_searches")}
            same_answer(space, ix.search_masked(q, words, k), want, (space, d, dtype, route, what, k))
            assert ix.stat("last_mask_rows") == int(visible.sum())
            host = keys_of(ix.search_keys_masked(q, words, k, ROW_BASE))
            same_keys(host, based(want, ROW_BASE), (space, d, dtype, route, what, k, "keys"))
            dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
            dev = keys_of(ix.search_keys_masked_dev(q, dev_words, k, ROW_BASE))
            assert np.array_equal(host, dev), "the device form differs from the host form"
            same_answer(space, ix.search_masked_dev_tensors(q, dev_words, k), want, (space, d, dtype, route, what, k, "dev"))
            after = {key: ix.stat(key) for key in before}
            assert after["masked_searches"] == before["masked_searches"] + 4
            assert after["masked_dev_searches"] == before["masked_dev_searches"] + 2
            moved = (after["mask_list_searches"] - before["mask_list_searches"], after["mask_dense_searches"] - before["mask_dense_searches"])
            assert moved == ((4, 0) if route == LIST else (0, 4)), ("the search left its route", route, moved)
            return want

        at128 = {}
        for k in ks_desc():
            for name, mask in (("half", half), ("upper", upper)):
                want = run(mask, k, name)
                at128.setdefault(name, want)
                assert np.array_equal(want, at128[name][:, :k])
            rows = kb.unpack(space, want[:1])[1][0]                          # upper, the plateau query
            clones = c.plateau[70:] if dead is None else c.plateau[70:][live[c.plateau[70:]]]
            head = np.concatenate([c.best[live[c.best]], clones])            # (at most 73 rows: a larger k goes on below the plateau)
            assert np.array_equal(rows[: len(head)], head[:k])
            for m in (k - 1, k, k + 1):                                      # exactly m visible rows
                mask = np.zeros(c.n, dtype=bool)
                if m:
                    mask[order[live[order]][:m]] = True
                    want = run(mask, k, ("visible", m))
                    assert ((want != 0).sum(axis=1) == min(m, k)).all()
        assert ix.stat("filter_passes") == 0
        ix.close()


# ---- 4. IVF ----------------------------------------------------------------------------------------------------------------------
NLIST = 16
EMPTY_LIST, SHORT_LIST = 3, 11
IVF_FORMS = [(64, "f32"), (768, "f32"), (1024, "f16"), (1536, "f32")]
IVF_CASES = [(s, d, t) for d, t in IVF_FORMS for s in SPACES3]


def ivf_layout(c):
    """(assign, perm, offsets, centroids): list EMPTY_LIST empty, SHORT_LIST 40 rows, the plateau over lists 0, 1 and 2, whose
    centroids lie around the plateau query (it probes them first); SHORT_LIST's centroid is the near-duplicate query, so that
    query's first probe holds fewer rows than k.  The test assigns the rows: the layout need not be a good clustering."""
    rng = np.random.default_rng(31 + c.d)
    others = np.delete(np.arange(NLIST), [EMPTY_LIST, SHORT_LIST])
    assign = rng.choice(others, size=c.n)
    ordinary = np.ones(c.n, dtype=bool)
    ordinary[c.planted] = False
    assign[np.flatnonzero(ordinary)[:: c.n // 40][:40]] = SHORT_LIST
    assign[c.plateau] = np.arange(kb.NPLATEAU) % 3
    assign[c.best] = [0, 1, 2]
    sizes = np.bincount(assign, minlength=NLIST)
    assert sizes[EMPTY_LIST] == 0 and 0 < sizes[SHORT_LIST] < 63
    perm = np.argsort(assign, kind="stable").astype(np.int64)
    offsets = np.zeros(NLIST + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes)
    cent = rng.standard_normal((NLIST, c.d)).astype(np.float32)
    cent[:3] = c.queries[kb.PLATEAU] + np.float32(0.1) * cent[:3]
    cent[SHORT_LIST] = c.queries[kb.NEAR]
    return assign, perm, offsets, cent


@functools.lru_cache(maxsize=None)
def ivf_reference(space, d, dtype):
    """(layout, probed [NQ, NLIST]: the lists by exact centroid score, best first)"""
    c = corpus(space, N_MASK, d, dtype)
    layout = ivf_layout(c)
    cent = layout[3]
    if space == "cosine":
        from oracle import knn_oracle as o

        stored_c = o.normalize_rows(cent)
    else:
        from tests import _space_reference as sr

        stored_c = sr.stored(cent, "f32")
    words = kb.score_words(space, stored_c, "f32", c.qprep)
    probed = kb.unpack(space, kb.top_keys(words, np.ones(NLIST, dtype=bool), NLIST))[1]
    return layout, probed


def ivf_want(c, assign, probed, qidx, nprobe, k, allowed=None):
    in_lists = np.zeros((kb.NQ, NLIST), dtype=bool)
    np.put_along_axis(in_lists, probed[:, :nprobe], True, axis=1)
    member = in_lists[:, assign]
    if allowed is not None:
        member = member & allowed[None, :]
    return kb.top_keys(c.score_word, member, k)[qidx]


@pytest.mark.parametrize("space,d,dtype", IVF_CASES, ids=[f"{s}-{d}-{t}" for s, d, t in IVF_CASES])
def test_ivf(env, space, d, dtype):
    torch, Index, ivf = env
    c = corpus(space, N_MASK, d, dtype)
    (assign, perm, offsets, cent), probed = ivf_reference(space, d, dtype)
    ix = open_index(Index, c, {"filter": 0, **({} if space == "cosine" else {"space_ivf": 1})})
    t = [torch.from_numpy(a).to(ix.device) for a in (cent, perm, offsets)]
    native.check(native.load().codd_knn_ivf_install(ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), ix._stream()), "codd_knn_ivf_install")

    def run(qidx, nprobe, k, allowed=None, what=""):
        want = ivf_want(c, assign, probed, qidx, nprobe, k, allowed)
        q = c.queries[qidx]
        got = keys_of(ivf.search_ivf_keys(ix, q, k, nprobe, ROW_BASE, allow=allowed))
        same_keys(got, based(want, ROW_BASE), (space, d, dtype, "ivf", len(qidx), nprobe, k, what))
        same_answer(space, ivf.search_ivf(ix, q, k, nprobe, allow=allowed), want, (space, d, dtype, "ivf", len(qidx), nprobe, k, what))
        return got, want

    # the per-pair scan
    ix.set_option("ivf_share", 0)
    shared0 = ix.stat("ivf_shared_searches")
    for B in (1, 9):
        qidx = c.batch(B)
        for nprobe in (1, 8, 16):
            at128 = None
            for k in ks_desc():
                got, want = run(qidx, nprobe, k)
                at128 = got if k == 128 else at128
                assert np.array_equal(got, at128[:, :k])
                if nprobe == NLIST:          # exhaustive probe: the flat search bit for bit
                    assert np.array_equal(got, based(top_all(space, N_MASK, d, dtype)[qidx][:, :k], ROW_BASE))
                    assert np.array_equal(got, keys_of(ix.search_keys(c.queries[qidx], k, ROW_BASE)))
    assert ix.stat("ivf_shared_searches") == shared0
    # a probe set that holds fewer than k rows pads: the near-duplicate query's first probe is the short list
    assert probed[kb.NEAR, 0] == SHORT_LIST and set(probed[kb.PLATEAU, :3].tolist()) == {0, 1, 2}
    m = int((assign == SHORT_LIST).sum())
    for k in ks_desc():
        got, want = run(np.array([kb.NEAR, kb.NEAR, kb.PLATEAU]), 1, k, what="short list")
        assert ((want[:2] != 0).sum(axis=1) == min(m, k)).all()
    # the list-sharing scan: 256 queries x 8 lists = 2,048 pairs, half of the batch the plateau query
    ix.set_option("ivf_share", 1)
    qidx = c.batch(256, half_plateau=True)
    shares = 0
    for k in ks_desc():
        before = ix.stat("ivf_shared_searches")
        run(qidx, 8, k, what="shared")
        shares += ix.stat("ivf_shared_searches") - before
    assert shares == 2 * len(KS), ("the batch did not share lists", shares)
    # under a mask and tombstones, at the slot boundary
    allow = np.random.default_rng(5).random(c.n) < 0.5
    allow[c.plateau[:70]] = False
    dead = dead_rows(c)
    ix.delete(np.flatnonzero(dead))
    before = ix.stat("ivf_masked_searches")
    for k in (64, 65):
        for B in (9, 256):
            qidx = c.batch(B, half_plateau=B == 256)
            want = ivf_want(c, assign, probed, qidx, 8, k, allow & ~dead)
            words = kb.words_of(allow)
            host = keys_of(ix.ivf_search_keys_masked(c.queries[qidx], words, k, 8, ROW_BASE))
            dev = keys_of(ix.ivf_search_keys_masked_dev(c.queries[qidx], torch.from_numpy(words.view(np.int32)).to(ix.device), k, 8, ROW_BASE))
            same_keys(host, based(want, ROW_BASE), (space, d, dtype, "ivf masked", B, k))
            assert np.array_equal(host, dev)
    assert ix.stat("ivf_masked_searches") == before + 8
    ix.close()


# ---- 5. the filter legs ----------------------------------------------------------------------------------------------------------
N_SMALL, N_LARGE, D_FILTER = 33_301, 66_003, 384                            # 131 and 258 tiles of 256 rows
KS_SMALL, KS_LARGE = tuple(k for k in KS if k <= 65), (127, 128)
GEMM8 = {"family": "GEMM", "nbq": 1, "el": 1, "res": 1}
PROGRAMS = [
    # id, B, options, the program last_pass must name, fused finalize + fallback possible (k <= 64)
    ("gemm8-resident", 20, {}, GEMM8, False),
    ("gemm8-staged", 20, {"resident_q": 0}, {**GEMM8, "res": 0}, False),
    ("tile-nbq4", 100, {}, {"family": "TILE", "nbq": 4, "el": 1}, True),
    ("tile-nbq8", 256, {}, {"family": "TILE", "nbq": 8, "el": 1}, True),
    ("tilef16", 256, {"shadow8": 0}, {"family": "TILE_F16", "nbq": 8, "el": 0}, True),
    ("gemm16", 20, {"shadow8": 0}, {"family": "GEMM", "nbq": 1, "el": 0}, True),
]


def filter_run(ix, c, top, qidx, k, program, what):
    before = ix.stat("filter_passes")
    want = top[qidx][:, :k]
    same_answer("cosine", ix.search(c.queries[qidx], k), want, what)
    assert ix.stat("filter_passes") == before + 1, ("the search did not take the filter leg", what)
    lp = ix.last_pass(keys_per_query=1, want_bmeta=False)
    ran = {key: lp[key] for key in program}
    assert ran == program and (lp["nq"], lp["k"], lp["n"]) == (len(qidx), k, c.n), ("another program ran", what, ran)
    # with these options the sample is min(max(64, 4k) in whole rounds of workgroups, ntiles): every tile here, and at least 2k
    ntiles = (c.n + fs.TILE - 1) // fs.TILE
    assert (lp["sample_tiles"], lp["sample_stride"]) == fs.sample_geometry(ntiles, k, bool(lp["el"]), lp["nbq"], ix.stat("num_cus")), what
    assert lp["sample_tiles"] >= 2 * k, what
    return lp


@pytest.mark.parametrize("n,ks", [(N_SMALL, KS_SMALL), (N_LARGE, KS_LARGE)], ids=["131-tiles", "258-tiles"])
@pytest.mark.parametrize("name,B,options,program,fusable", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_filter_leg(env, name, B, options, program, fusable, n, ks):
    _, Index, _ = env
    c = corpus("cosine", n, D_FILTER, "f32")
    top = top_all("cosine", n, D_FILTER, "f32")
    ix = open_index(Index, c, {**fs.BASE_OPTIONS, **options})
    qidx = c.batch(B)
    for k in ks_desc(ks):
        for fuse in (1, 0) if k <= 64 else (1,):
            ix.set_option("fuse_fallback", fuse)
            ix.set_option("hit_cap", 131_072)
            filter_run(ix, c, top, qidx, k, program, (name, n, k, "fuse", fuse))
            got = keys_of(ix.search_keys(c.queries[qidx], k, ROW_BASE))
            same_keys(got, based(top[qidx][:, :k], ROW_BASE), (name, n, k, "keys"))
            # Candidate lists cut short: the queries whose raw counter passes the cap are answered by the exact-scan fallback, merged
            # behind finalize, the others by finalize; the bits stay.  The zero query's list holds every row, so it overflows under
            # either cap.  Under a cap of 64 the plateau query overflows as well from k = 4 on (its 143 planted rows reach any
            # threshold that an answer of 4 .. 143 rows allows), and from k = 65 on EVERY query does (an answer needs k candidates):
            # "fewer than B" is asserted where counting allows it, k <= 2 (a threshold at the best sampled row leaves a no-tie query
            # a handful of candidates).  Under a cap of 4,096 finalize and the fallback share the batch at every k.
            for cap in (64, 4_096):
                ix.set_option("hit_cap", cap)
                fb0 = ix.stat("fallback_queries")
                lp = filter_run(ix, c, top, qidx, k, program, (name, n, k, "hit_cap", cap, "fuse", fuse))
                fb = ix.stat("fallback_queries") - fb0
                over = int((lp["hit_counts"].astype(np.int64) > cap).sum())
                print(name, n, "k", k, "fuse", fuse, "hit_cap", cap, "fallback_queries", fb, "of", B, "fb_count", lp["fb_count"],
                      "counters of the first 8 queries", lp["hit_counts"][:8].tolist())
                assert lp["hit_cap"] == cap and lp["hit_counts"][kb.ZERO] == c.n and fb == over and 1 <= fb <= B
                if cap == 64:
                    assert k < 4 or lp["hit_counts"][kb.PLATEAU] > 64
                    assert fb == B if k > 64 else (fb < B or k > 2)
                else:
                    assert fb < B, "finalize and the fallback must share the batch"
                # the fused launch derives the fallback queue from the counters and writes none; finalize as its own launch writes it
                fused = fusable and fuse == 1 and k <= 64
                assert lp["flags"][1] == 1 and lp["fb_count"] == (0 if fused else over), ("fused" if fused else "two launches", name, k)
    # the leg ends where the sample has fewer than 2k tiles: ntiles >= 2k, 131 tiles: 65 filters, 66 scans
    ix.set_option("hit_cap", 131_072)
    if n == N_SMALL:
        before = (ix.stat("filter_passes"), ix.stat("scan_launches"))
        same_answer("cosine", ix.search(c.queries[qidx], 66), top[qidx][:, :66], (name, "k = 66"))
        assert (ix.stat("filter_passes"), ix.stat("scan_launches")) == (before[0], before[1] + 1), "k = 66 over 131 tiles must be a scan"
        # tombstones on the lowest clone and on one of the 3 best
        dead = np.zeros(c.n, dtype=bool)
        dead[[c.plateau[0], c.best[1]]] = True
        ix.delete(np.flatnonzero(dead))
        live_top = kb.top_keys(c.score_word, ~dead)
        for k in (64, 65):
            filter_run(ix, c, live_top, qidx, k, program, (name, "tombstones", k))
    ix.close()


def test_filter_leg_with_a_shared_out_finalize(env):
    """8 queries: each query's re-scoring is shared out over 16 workgroups, whose 16 lists of k are merged"""
    _, Index, _ = env
    c = corpus("cosine", N_SMALL, D_FILTER, "f32")
    top = top_all("cosine", N_SMALL, D_FILTER, "f32")
    ix = open_index(Index, c, fs.BASE_OPTIONS)
    qidx = c.batch(8)
    for k in (63, 64, 65):
        filter_run(ix, c, top, qidx, k, GEMM8, ("shared out", k))
        assert ix.stat("last_finalize_parts") == 16
    ix.close()


# ---- 6. the one-launch small batch ---------------------------------------------------------------------------------------------------
def test_small_batch(env):
    _, Index, _ = env
    c = corpus("cosine", N_SMALL, D_FILTER, "f32")
    top = top_all("cosine", N_SMALL, D_FILTER, "f32")
    ix = open_index(Index, c, {**fs.BASE_OPTIONS, "small_batch_max": 1})
    for qn in (kb.PLATEAU, kb.NOTIE, kb.ZERO, kb.NEAR):
        qidx = np.array([qn])
        for k in (65, 64, 63, 16, 1):
            before = (ix.stat("small_batch_passes"), ix.stat("filter_passes"))
            same_answer("cosine", ix.search(c.queries[qidx], k), top[qidx][:, :k], ("small batch", qn, k))
            moved = (ix.stat("small_batch_passes") - before[0], ix.stat("filter_passes") - before[1])
            assert moved == ((1, 0) if k <= 64 else (0, 1)), ("small_batch_kernel is for k <= 64 only", qn, k, moved)
    ix.close()


# ---- 7. the opt-in int8 leg of ip and l2 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["ip", "l2"])
@pytest.mark.parametrize("n,ks", [(N_SMALL, (16, 17, 63, 64, 65)), (N_LARGE, (128,))], ids=["131-tiles", "258-tiles"])
def test_space_filter(env, space, n, ks):
    _, Index, _ = env
    c = corpus(space, n, D_FILTER, "f32")
    top = top_all(space, n, D_FILTER, "f32")
    ix = open_index(Index, c, {**fs.BASE_OPTIONS, "space_filter": 1})
    for B in (24, 100):
        qidx = c.batch(B)
        for k in ks_desc(ks):
            before = (ix.stat("filter_passes"), ix.stat("shadow8_passes"), ix.stat("scan_launches"))
            same_answer(space, ix.search(c.queries[qidx], k), top[qidx][:, :k], (space, n, B, k))
            after = (ix.stat("filter_passes"), ix.stat("shadow8_passes"), ix.stat("scan_launches"))
            assert after == (before[0] + 1, before[1] + 1, before[2]), ("the search did not take the int8 leg", space, B, k)
            lp = ix.last_pass(keys_per_query=1, want_bmeta=False)
            assert (lp["family"], lp["el"], lp["sqd"], lp["k"]) == ("GEMM", 1, int(space == "l2"), k)
        if n == N_SMALL:
            before = (ix.stat("filter_passes"), ix.stat("scan_launches"))
            same_answer(space, ix.search(c.queries[qidx], 66), top[qidx][:, :66], (space, n, B, 66))
            assert (ix.stat("filter_passes"), ix.stat("scan_launches")) == (before[0], before[1] + 1), "k = 66 over 131 tiles must be a scan"
    ix.close()


# ---- 8. two shards -----------------------------------------------------------------------------------------------------------------
CUT = 2_605


@pytest.mark.parametrize("space", SPACES3)
def test_two_shards_merge_to_the_whole_index(env, space):
    torch, Index, _ = env
    from codd_query_engine_amd.knn_index import merge_keys, merge_shards

    d, dtype = 768, "f32"
    c = corpus(space, N_MASK, d, dtype)
    top = top_all(space, N_MASK, d, dtype)
    assert (c.plateau < CUT).sum() >= 3 and (c.plateau >= CUT).sum() >= 3, "the plateau must cross the cut"
    shards = [open_index(Index, c, {"filter": 0}, rows=np.arange(0, CUT)), open_index(Index, c, {"filter": 0}, rows=np.arange(CUT, c.n))]
    lib = native.load()
    qidx = c.batch(9)
    q = c.queries[qidx]
    for k in ks_desc():
        want = based(top[qidx][:, :k], ROW_BASE)
        parts = [shards[0].search_keys(q, k, ROW_BASE), shards[1].search_keys(q, k, ROW_BASE + CUT)]
        keys, dist, rows = merge_keys(torch.cat(parts, dim=1), k, space=space)
        same_keys(keys_of(keys), want, (space, "merge_keys", k))
        same_answer(space, (dist, rows - ROW_BASE), top[qidx][:, :k], (space, "merge_keys", k))
        keys2, dist2, rows2 = merge_shards(torch.cat(parts, dim=0), 2, k, space=space)
        assert torch.equal(keys2, keys) and torch.equal(rows2, rows) and np.array_equal(kb.bits(dist2.cpu().numpy()), kb.bits(dist.cpu().numpy()))
        if space == "cosine":      # the entry points without a metric are the cosine ones
            both = torch.cat(parts, dim=1).contiguous()
            out = [torch.empty((9, k), dtype=t, device=both.device) for t in (torch.int64, torch.float32, torch.int64)]
            native.check(lib.codd_knn_merge_keys(0, both.data_ptr(), 9, 2 * k, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), shards[0]._stream()), "codd_knn_merge_keys")
            assert torch.equal(out[0], keys) and torch.equal(out[2], rows) and torch.equal(out[1], dist)
            gathered = torch.cat(parts, dim=0).contiguous()
            native.check(lib.codd_knn_merge_shards(0, gathered.data_ptr(), 2, 9, k, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), shards[0]._stream()), "codd_knn_merge_shards")
            assert torch.equal(out[0], keys) and torch.equal(out[2], rows) and torch.equal(out[1], dist)
    for ix in shards:
        ix.close()


# ---- k = 0 and k = 129 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_k_out_of_range_is_einval_and_the_next_search_is_right(env, space):
    torch, Index, ivf = env
    from codd_query_engine_amd.knn_index import merge_keys, merge_shards

    d, dtype = 64, "f32"
    c = corpus(space, N_MASK, d, dtype)
    top = top_all(space, N_MASK, d, dtype)
    (assign, perm, offsets, cent), probed = ivf_reference(space, d, dtype)
    ix = open_index(Index, c, {"filter": 0, **({} if space == "cosine" else {"space_ivf": 1})})
    t = [torch.from_numpy(a).to(ix.device) for a in (cent, perm, offsets)]
    native.check(native.load().codd_knn_ivf_install(ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), ix._stream()), "codd_knn_ivf_install")
    ix.set_scopes(np.arange(c.n, dtype=np.int64), np.ones(c.n, dtype=np.uint32))
    qidx = c.batch(4)
    q = c.queries[qidx]
    ones = np.ones(c.n, dtype=bool)
    words = kb.words_of(ones)
    dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
    scopes = np.ones(4, dtype=np.uint32)
    some_keys = ix.search_keys(q, 64)
    calls = {
        "search": lambda k: ix.search(q, k),
        "search_keys": lambda k: ix.search_keys(q, k),
        "scoped": lambda k: ix.search_scoped(q, scopes, k),
        "scoped keys": lambda k: ix.search_keys_scoped(q, scopes, k),
        "masked host": lambda k: ix.search_masked(q, words, k),
        "masked device": lambda k: ix.search_masked_dev_tensors(q, dev_words, k),
        "ivf": lambda k: ivf.search_ivf(ix, q, k, 8),
        "ivf keys": lambda k: ivf.search_ivf_keys(ix, q, k, 8),
        "ivf masked host": lambda k: ix.ivf_search_masked_tensors(q, words, k, 8),
        "ivf masked device": lambda k: ix.ivf_search_masked_dev_tensors(q, dev_words, k, 8),
        "merge_keys": lambda k: merge_keys(some_keys, k, space=space),
        "merge_shards": lambda k: merge_shards(some_keys, 2, k, space=space),
    }
    for name, call in calls.items():
        for k in (0, 129):
            with pytest.raises(native.NativeLibraryError, match=EINVAL):
                call(k)
            for kk in (64, 65):
                same_answer(space, ix.search(q, kk), top[qidx][:, :kk], ("after", name, k, kk))
    lib = native.load()
    out = [torch.empty((4, 129), dtype=dt, device=ix.device) for dt in (torch.int64, torch.float32, torch.int64)]
    for k in (0, 129):          # the cosine merges without a metric argument
        assert lib.codd_knn_merge_keys(0, some_keys.data_ptr(), 4, 64, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ix._stream()) == -22
        assert lib.codd_knn_merge_shards(0, some_keys.data_ptr(), 2, 2, 64, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ix._stream()) == -22
    # every entry point still answers: one valid call each, against the reference
    same_answer(space, ix.search_scoped(q, scopes, 65), top[qidx][:, :65], "scoped after the refusals")
    same_answer(space, ix.search_masked(q, words, 65), top[qidx][:, :65], "masked after the refusals")
    same_answer(space, ivf.search_ivf(ix, q, 65, NLIST), top[qidx][:, :65], "ivf after the refusals")
    ix.close()
