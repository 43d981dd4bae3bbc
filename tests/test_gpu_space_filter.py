"""The opt-in int8 filter leg of an ip or l2 index on the GPU.  Two things are held:

  * the bound: the values the leg filters with (approx_scores) lie within filter_slack's eps(q) of the fp64 score of every stored
    row, for the inputs of tests/test_space_filter_bound.py;
  * the answers: ids and the bits of every distance equal tests/_space_reference.py — what the exact scan returns — for the first
    16 queries of every batch and every planted query, while the stats show that the leg ran (and, option off, that it did not).
"""

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _space_filter_reference as fr
from tests import _space_reference as sr

pytestmark = pytest.mark.gpu

N = 6144          # 24 tiles of 256 rows: the sample holds 2k tiles at k = 10
TOP = native.MAX_GLOBAL_ROW
LEG_STATS = ("filter_passes", "shadow8_passes", "i8v2_passes", "shadow16_builds", "scan_launches")


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def build(Index, space, dtype, raw, on=1, **options):
    ix = Index(raw.shape[1], dtype=dtype, space=space)
    for key, value in options.items():
        ix.set_option(key, value)
    ix.set_option("space_filter", on)
    ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw, normalize=False)
    return ix


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    (gd, gr), (wd, wr) = got, want
    gd, gr = np.asarray(gd), np.asarray(gr)
    assert np.array_equal(gr, wr), (what, "rows", np.flatnonzero((gr != wr).any(axis=1))[:8])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")


def gaussian(n, d, B, seed):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = (1.3 * rng.standard_normal((B, d))).astype(np.float32)
    return raw, q


def stats(ix):
    return {key: ix.stat(key) for key in LEG_STATS}


# ---- d. the bound on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("d", [200, 768])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_filter_values_within_filter_slack_of_the_reference(Index, space, d, dtype):
    n, B = 2048, 24
    for kind in fr.KINDS:
        raw, q = fr.inputs(kind, n, B, d, dtype)
        ix = build(Index, space, dtype, raw)
        model = fr.Model(space, raw, dtype, q)
        assert np.array_equal(ix.read_rows(), sr.stored(raw, dtype))
        eps = ix.filter_slack(q).cpu().numpy().astype(np.float64)
        got = ix.approx_scores(q)[:B].cpu().numpy().astype(np.float64)
        err = np.abs(got - model.exact64())
        print(space, d, dtype, kind, "largest error / eps(q):", (err / eps[:, None]).max(), "eps:", eps.min(), "..", eps.max())
        assert np.isfinite(eps).all() and (eps > 0).all()
        assert (err <= eps[:, None]).all(), (kind, np.argwhere(err > eps[:, None])[:4])
        # the device's slack is the model's (the fp32 sums run in another order: far below one part in a thousand)
        assert np.allclose(eps, model.slack(), rtol=1e-3, atol=0), (kind, eps[:4], model.slack()[:4])
        ix.close()


def test_filter_slack_of_a_cosine_index_is_todays_eps(Index):
    raw, q = gaussian(2048, 768, 24, seed=3)
    ix = Index(768, dtype="f32")
    ix.upsert(np.arange(2048, dtype=np.int64), raw)
    eps = ix.filter_slack(q).cpu().numpy()
    want = fr.Model("cosine", raw, "f32", q).slack()
    assert np.allclose(eps, want, rtol=1e-3, atol=0), (eps[:4], want[:4])
    got = ix.approx_scores(q)[:24].cpu().numpy().astype(np.float64)
    exact = o.normalize_rows(q).astype(np.float64) @ o.normalize_rows(raw).astype(np.float64).T
    assert (np.abs(got - exact) <= eps[:, None]).all()
    ix.close()


def test_the_debug_entry_points_refuse_without_the_option(Index):
    raw, q = gaussian(2048, 64, 40, seed=6)
    for space in sr.SPACES:
        ix = build(Index, space, "f32", raw, on=0)
        for call in (lambda: ix.approx_scores(q[:4]), lambda: ix.filter_slack(q[:4])):
            with pytest.raises(native.NativeLibraryError):
                call()
        ix.set_option("space_filter", 1)
        with pytest.raises(native.NativeLibraryError):
            ix.approx_scores(q)                            # 40 queries: more than the DUMP form takes
        assert ix.filter_slack(q).shape[0] == 40
        ix.close()


# ---- e. exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("d", [200, 768])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_every_batch_size_equals_the_reference_and_takes_the_leg(Index, space, d, dtype):
    raw, q = gaussian(N, d, 300, seed=d + len(dtype))
    ix = build(Index, space, dtype, raw)
    want = sr.Reference(space, raw, dtype, q[:16]).topk(9, 10)[1:], sr.Reference(space, raw, dtype, q[:16]).topk(16, 10)[1:]
    for B in (9, 40, 100, 256, 300):
        before = stats(ix)
        dist, rows = ix.search(q[:B], 10)
        m = min(B, 16)
        same((dist[:m], rows[:m]), want[0] if m == 9 else want[1], (space, dtype, d, B))
        after = stats(ix)
        passes = (B + 255) // 256
        assert after["filter_passes"] - before["filter_passes"] == passes and after["shadow8_passes"] - before["shadow8_passes"] == passes, (B, before, after)
        for key in ("i8v2_passes", "shadow16_builds", "scan_launches"):
            assert after[key] == before[key], (B, key)
    assert ix.stat("fallback_queries") == 0, "Gaussian data: no query overflows its candidate list"
    assert ix.stat("filter_hits") > 0 and ix.stat("filter_survivors") >= 10 * 705
    # option off: the same index answers identically through the scan
    ix.set_option("space_filter", 0)
    before = stats(ix)
    dist, rows = ix.search(q[:100], 10)
    same((dist[:16], rows[:16]), want[1], (space, dtype, d, "off"))
    after = stats(ix)
    assert after["filter_passes"] == before["filter_passes"] and after["scan_launches"] == before["scan_launches"] + 1
    ix.close()


# ---- f. hard inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", sr.SPACES)
def test_norms_over_six_decades_and_zero_vectors(Index, space):
    d, B = 200, 24
    raw, q = fr.inputs("gaussian_decades", N, B, d)
    raw[[3, 77, 4000]] = 0.0
    raw[9, 5], raw[5000, 0] = np.nan, np.inf                # stored as zero rows
    q[2], q[5, 7] = 0.0, np.nan                             # the zero query, twice
    ix = build(Index, space, "f32", raw)
    ref = sr.Reference(space, raw, "f32", q)
    same(ix.search(q, 10), ref.topk(B, 10)[1:], (space, "decades"))
    assert ix.stat("filter_passes") == 1 and ix.stat("scan_launches") == 0
    # deleted rows, then the dense route of a masked search with half the rows allowed, then keys with a row base
    top = ref.topk(B, 10)[2]
    gone = np.unique(np.concatenate([top[:, :2].ravel(), np.arange(600, 700)]))
    live = np.ones(N, dtype=bool)
    live[gone] = False
    ix.delete(gone)
    same(ix.search(q, 10), ref.topk(B, 10, allow=live)[1:], (space, "after delete"))
    allow = np.random.default_rng(1).random(N) < 0.5
    ix.set_option("mask_route", 2)
    same(ix.search_masked(q, allow, 10), ref.topk(B, 10, allow=allow & live)[1:], (space, "dense mask"))
    assert ix.stat("mask_dense_searches") == 1
    base = TOP - (N - 1)
    keys = ix.search_keys(q, 10, base).cpu().numpy().view(np.uint64)
    assert np.array_equal(keys, ref.topk(B, 10, allow=live, row_base=base)[0])
    assert ix.stat("filter_passes") == 4 and ix.stat("scan_launches") == 0, "all four searches took the leg"
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_near_copies_of_a_query_one_ulp_apart(Index, space):
    d, B = 768, 16
    raw, q = gaussian(N, d, B, seed=21)
    q[4] = raw[123]
    ids = np.arange(2000, 2300)
    raw[ids] = q[0]
    for j, r in enumerate(ids):
        if r != 2150:                                       # row 2150 stays the exact copy
            raw[r, j % d] = np.nextafter(raw[r, j % d], np.float32(np.inf if j % 2 else -np.inf))
    ix = build(Index, space, "f32", raw)
    ref = sr.Reference(space, raw, "f32", q)
    same(ix.search(q, 10), ref.topk(B, 10)[1:], (space, "near copies"))
    if space == "l2":
        dist, rows = ix.search(q, 10)
        assert rows[0, 0] == 2150 and bits(dist)[0, 0] == 0, "the exact copy: distance +0.0"
        assert rows[4, 0] == 123 and bits(dist)[4, 0] == 0
        tied = rows[0][dist[0] == dist[0, 1]]
        assert (np.diff(tied) > 0).all(), "equal distances: the lower row first"
    assert ix.stat("scan_launches") == 0
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_a_larger_row_appended_after_the_first_search(Index, space):
    d, B = 200, 24
    raw, q = gaussian(N, d, B, seed=33)
    ix = build(Index, space, "f32", raw)
    same(ix.search(q, 10), sr.Reference(space, raw, "f32", q).topk(B, 10)[1:], (space, "before"))
    eps0 = ix.filter_slack(q).cpu().numpy()
    big = (1e3 * raw[:3]).astype(np.float32)
    big[1] = -big[1]
    ix.upsert(np.arange(N, N + 3, dtype=np.int64), big, normalize=False)
    raw2 = np.concatenate([raw, big])
    eps1 = ix.filter_slack(q).cpu().numpy()
    assert (eps1 > 100 * eps0).all(), "R and eps_r follow the rows stored now"
    same(ix.search(q, 10), sr.Reference(space, raw2, "f32", q).topk(B, 10)[1:], (space, "after"))
    assert ix.stat("shadow8_builds") == 2 and ix.stat("scan_launches") == 0
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_two_list_slots_per_lane(Index, space):
    n, d, B = 51200, 64, 24                                 # 200 tiles = 2k at k = 100
    raw, q = gaussian(n, d, B, seed=41)
    ix = build(Index, space, "f32", raw)
    dist, rows = ix.search(q, 100)
    same((dist[:8], rows[:8]), sr.Reference(space, raw, "f32", q[:8]).topk(8, 100)[1:], (space, "k = 100"))
    assert ix.stat("filter_passes") == 1 and ix.stat("scan_launches") == 0
    ix.close()


# ---- g. the fallback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("B", [24, 100])
def test_queries_over_the_hit_cap_fall_back_and_stay_exact(Index, space, B):
    """One giant row makes eps(q) larger than every score: every row is a hit, far more than the 64 candidates a query may
    keep.  B = 100 takes the fused finalize where ip may (l2: the listed squared-distance scan either way)."""
    raw, q = fr.inputs("one_giant_row", N, B, 200)
    ix = build(Index, space, "f32", raw, hit_cap=64)
    dist, rows = ix.search(q, 10)
    same((dist[:16], rows[:16]), sr.Reference(space, raw, "f32", q[:16]).topk(16, 10)[1:], (space, B, "fallback"))
    assert ix.stat("fallback_queries") > 0 and ix.stat("filter_passes") == 1 and ix.stat("scan_launches") == 0
    ix.close()


# ---- h. not vacuous -------------------------------------------------------------------------------------------------------------
def test_not_vacuous(Index):
    """Unit rows, unit queries: the three bounds differ by the small gamma terms only (l2: value and slack both doubled), so the ip
    and the l2 leg must let through about what the cosine int8 filter does with its first-generation kernel — under twice that."""
    d, B = 768, 64
    rng = np.random.default_rng(5)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)  # noqa: E731
    raw, q = unit(rng.standard_normal((N, d))), unit(rng.standard_normal((B, d)))
    hits = {}
    cos = Index(d, dtype="f32")
    cos.set_option("i8v2", 0)
    cos.upsert(np.arange(N, dtype=np.int64), raw)
    cos.search(q, 10)
    assert cos.stat("shadow8_passes") == 1
    hits["cosine"] = cos.stat("filter_hits")
    cos.close()
    for space in sr.SPACES:
        ix = build(Index, space, "f32", raw)
        ix.search(q, 10)
        assert ix.stat("shadow8_passes") == 1
        hits[space] = ix.stat("filter_hits")
        ix.close()
    print("filter_hits of 64 unit queries over 6,144 unit rows:", hits)
    assert 0 < hits["ip"] < 2 * hits["cosine"] and 0 < hits["l2"] < 2 * hits["cosine"], hits
