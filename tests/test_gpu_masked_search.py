"""Masked search on the GPU, through the C ABI (codd_knn_search_masked).  The expected answer of every query is
the oracle's search over the rows that are allowed AND live (row order kept, so "ties -> lower row" carries over), its indices
mapped back to row slots.  Every comparison is bit for bit on row ids and fp32 distances, padding included: no tolerance, no
query left out.  The route is forced with "mask_route" and confirmed through the masked-search stats and the existing path
stats; the shapes are the smallest at which each path exists (as in test_gpu_deletes.py)."""

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, native
from oracle import knn_oracle as o
from tests._deleting_oracle_engine import live_reference
from tests._masked_oracle_engine import MaskedOracleEngine
from tests.test_gpu_deletes import always_filter, expected_keys, planted, stored

pytestmark = pytest.mark.gpu

LIST, DENSE = 1, 2


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex


def check(ix, rows_ref, dtype, visible, allow, q, k, route, what=""):
    """one masked search on `route` against the oracle over `visible` (= allowed and live); returns (dist, rows)"""
    ix.set_option("mask_route", route)
    before = (ix.stat("masked_searches"), ix.stat("mask_list_searches"), ix.stat("mask_dense_searches"))
    d_ref, r_ref = live_reference(rows_ref, dtype, np.flatnonzero(visible), o.normalize_rows(q), k)
    dist, rows = ix.search_masked(q, allow, k)
    bad = np.flatnonzero((rows != r_ref).any(axis=1))
    assert bad.size == 0, (what, dtype, q.shape, k, route, bad[:8], rows[bad[:1]], r_ref[bad[:1]])
    assert np.array_equal(dist, d_ref), (what, dtype, q.shape, k, route)
    m = int(visible.sum())
    assert ix.stat("last_mask_rows") == m and ix.stat("masked_searches") == before[0] + 1
    if m:
        assert (ix.stat("mask_list_searches"), ix.stat("mask_dense_searches")) == (before[1] + (route == LIST), before[2] + (route == DENSE)), what
    return dist, rows


# ------------------------------------------------------------------------------------------------------------------------
# the dense route through every family of the ordinary dispatch, under one adversarial mask: half of the rows at random; per
# query the best 5 of 10 planted near-duplicates disallowed (the threshold anchors and finalize's first k would all be
# disallowed rows); four whole leading tiles disallowed (tile 0 is always sampled); one disallowed row tying exactly with an
# allowed one
# ------------------------------------------------------------------------------------------------------------------------
PATHS = [
    # name, dtype, dim, n, B, filter forced on whatever the size, options, stat that must move
    ("scan", "f32", 768, 12_000, 8, False, {}, "scan_launches"),
    ("bf16_gemm", "f32", 768, 60_000, 40, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes"),
    ("f16_tile", "f32", 768, 40_000, 200, True, {"shadow8": 0}, "f16_tile_passes"),
    ("i8_gen1", "f32", 768, 60_000, 40, True, {"i8v2": 0}, "shadow8_passes"),
    ("i8_tile", "f32", 768, 40_000, 256, True, {}, "i8v2_passes"),
    ("i8_tile_half", "f32", 768, 40_000, 100, True, {}, "i8v2_passes"),
    ("fallback", "f32", 768, 40_000, 140, True, {"hit_cap": 16}, "mask_fallback_queries"),
    ("fallback_unfused", "f32", 768, 60_000, 40, True, {"hit_cap": 16}, "mask_fallback_queries"),
    ("wide_f32_1536", "f32", 1536, 40_000, 140, True, {}, "filter_passes"),
]


@pytest.mark.parametrize("name,dtype,dim,n,B,forced,options,moved", PATHS, ids=[p[0] for p in PATHS])
def test_dense_route_through_every_family(env, name, dtype, dim, n, B, forced, options, moved):
    _, Index = env
    rng = np.random.default_rng(len(name) * 1000 + dim + B)
    raw, q, slots = planted(rng, n, dim, B)
    free = np.setdiff1d(np.arange(2000, n), slots.ravel())
    a, b = int(free[10]), int(free[400])
    raw[b] = raw[a]                                   # an exact tie: the earlier row will be disallowed
    q[-1] = raw[a]
    ix = Index(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    if forced:
        always_filter(ix)
    for key, value in options.items():
        ix.set_option(key, value)
    rows_ref = stored(raw, dtype)
    allow = rng.random(n) < 0.5
    allow[slots[:, 5:].ravel()] = True
    allow[slots[:, :5].ravel()] = False
    allow[:1024] = False
    allow[a], allow[b] = False, True
    before, unmasked_counters = ix.stat(moved), (ix.stat("filter_hits"), ix.stat("filter_survivors"), ix.stat("fallback_queries"))
    dist, rows = check(ix, rows_ref, dtype, allow, allow, q, 10, DENSE, name)
    assert allow[rows[rows >= 0]].all()
    assert rows[-1, 0] == b and dist[-1, 0] == live_reference(rows_ref, dtype, np.array([a]), o.normalize_rows(q[-1:]), 1)[0][0, 0]
    # (which of two neighbouring planted rows scores higher is up to their noise: compared as sets, the oracle fixed the order above)
    assert (np.sort(rows[:-1, :5], axis=1) == np.sort(slots[:-1, 5:], axis=1)).all(), "the five allowed planted rows lead"
    assert ix.stat(moved) > before, (name, moved)
    assert (ix.stat("filter_hits"), ix.stat("filter_survivors"), ix.stat("fallback_queries")) == unmasked_counters, "the watch's counters stay out of it"
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# the list route: small masks, every instantiation family of mask_scan_kernel (narrow f32, 2-byte, wide 2-byte with two queries per
# work item), counts that are no multiple of 32 with garbage above the count in the last word
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim,n", [("f32", 768, 20_001), ("bf16", 384, 30_011), ("bf16", 4096, 6_005)], ids=["f32_768", "bf16_384", "bf16_4096"])
def test_list_route(env, dtype, dim, n):
    _, Index = env
    rng = np.random.default_rng(dim + n)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    rows_ref = stored(raw, dtype)
    assert n % 32 != 0
    scans = ix.stat("scan_launches")
    for share in (0.01, 0.0005):
        allow = np.zeros(n, dtype=bool)
        allow[rng.permutation(n)[: int(round(n * share))]] = True    # (below: never a whole number of 16-row workgroup steps)
        allow[n - 1] = True                                          # the last row of the ragged word
        if allow.sum() % 16 == 0:
            allow[np.flatnonzero(~allow)[0]] = True
        words = np.zeros((n + 31) // 32 * 32, dtype=bool)
        words[:n] = allow
        words[n:] = True                                             # garbage above count
        packed = np.packbits(words, bitorder="little").view("<u4")
        for B in (1, 5, 256):
            q = rng.standard_normal((B, dim)).astype(np.float32)
            q[0] = raw[np.flatnonzero(allow)[0]]
            k = 10 if B != 5 else 100                                # k = 100: two list slots per lane; above m at the small share
            dist, rows = check(ix, rows_ref, dtype, allow, packed if B != 1 else allow, q, k, LIST, f"{share} B={B}")
            hits = min(k, int(allow.sum()))
            assert (rows[:, :hits] >= 0).all() and (rows[:, hits:] == -1).all() and np.isinf(dist[:, hits:]).all()
            assert rows[0, 0] == np.flatnonzero(allow)[0]
    assert ix.stat("scan_launches") == scans and ix.stat("filter_passes") == 0, "the list route runs neither the scan nor a filter"
    ix.close()


def test_both_routes_return_identical_bits_and_so_does_the_rule(env):
    _, Index = env
    rng = np.random.default_rng(31)
    n, dim, B = 40_000, 768, 140
    raw, q, slots = planted(rng, n, dim, B)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    for share in (0.03, 0.8):
        allow = rng.random(n) < share
        allow[slots[:, ::2].ravel()] = True
        got = [check(ix, rows_ref, "f32", allow, allow, q, 10, route, f"share {share}") for route in (LIST, DENSE)]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        ix.set_option("mask_route", 0)                               # the rule: whichever it takes, the same bits
        counted = ix.stat("mask_list_searches") + ix.stat("mask_dense_searches")
        dist, rows = ix.search_masked(q, allow, 10)
        assert np.array_equal(dist, got[0][0]) and np.array_equal(rows, got[0][1])
        assert ix.stat("mask_list_searches") + ix.stat("mask_dense_searches") == counted + 1
    # 3 % of 40,000 rows leave fewer than 4k expected anchors among the sampled tiles: the rule takes the list; 80 % the dense route
    assert ix.stat("mask_list_searches") == 3 and ix.stat("mask_dense_searches") == 3
    ix.close()


def test_all_ones_all_zero_and_tombstones_under_the_mask(env):
    _, Index = env
    rng = np.random.default_rng(32)
    n, dim, B = 40_000, 768, 140
    raw, q, slots = planted(rng, n, dim, B)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    ones = np.ones(n, dtype=bool)
    d0, r0 = ix.search(q, 10)
    for route in (DENSE, LIST):
        dist, rows = check(ix, rows_ref, "f32", ones, ones, q, 10, route, "all ones")
        assert np.array_equal(dist, d0) and np.array_equal(rows, r0), "an all-ones mask returns the bits of search"
    launches = (ix.stat("scan_launches"), ix.stat("filter_passes"))
    for route in (DENSE, LIST):
        dist, rows = check(ix, rows_ref, "f32", ~ones, ~ones, q, 10, route, "all zero")
        assert (rows == -1).all() and np.isinf(dist).all()
    assert (ix.stat("scan_launches"), ix.stat("filter_passes")) == launches and ix.stat("last_mask_rows") == 0
    # tombstones first (1 %, among them each query's best planted row), then masks that allow dead rows
    dead = np.concatenate([rng.permutation(n)[: n // 100], slots[:, 0]])
    ix.delete(dead)
    live = ones.copy()
    live[dead] = False
    for share, route in ((0.5, DENSE), (0.02, LIST), (0.5, LIST)):
        allow = rng.random(n) < share
        allow[dead[::2]] = True                                      # allowed but dead
        dist, rows = check(ix, rows_ref, "f32", allow & live, allow, q, 10, route, f"tombstones {share}")
        assert not np.isin(rows, dead).any() and allow[rows].all()
    only_dead = np.zeros(n, dtype=bool)
    only_dead[dead] = True
    dist, rows = check(ix, rows_ref, "f32", only_dead & live, only_dead, q, 10, DENSE, "only dead rows allowed")
    assert (rows == -1).all()
    ix.close()


def test_search_keys_masked_with_a_row_base(env):
    _, Index = env
    rng = np.random.default_rng(33)
    n, dim, B, base = 40_000, 768, 140, 3_000_000
    raw, q, _ = planted(rng, n, dim, B)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    for share, route in ((0.5, DENSE), (0.01, LIST)):
        allow = rng.random(n) < share
        ix.set_option("mask_route", route)
        keys = ix.search_keys_masked(q, allow, 10, row_base=base).cpu().numpy().view(np.uint64)
        assert np.array_equal(keys, expected_keys(rows_ref, "f32", allow, q, 10, base)), route
    assert ix.stat("mask_dense_searches") == 1 and ix.stat("mask_list_searches") == 1
    ix.close()


def test_two_masks_on_two_streams(env):
    torch, Index = env
    rng = np.random.default_rng(34)
    n, dim, B = 40_000, 768, 64
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    q = torch.from_numpy(rng.standard_normal((B, dim)).astype(np.float32)).cuda()
    masks = [rng.random(n) < 0.5, rng.random(n) < 0.01]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = []
    for rnd in range(2):                                             # the second round reuses each stream's staging buffer
        for s, allow, route in zip(streams, masks, (DENSE, LIST)):
            ix.set_option("mask_route", route)
            with torch.cuda.stream(s):
                out.append(ix.search_masked_tensors(q, allow, 10))
    torch.cuda.synchronize()
    assert ix.stat("workspaces") >= 2
    for i, (dist, rows) in enumerate(out):
        d_ref, r_ref = live_reference(rows_ref, "f32", np.flatnonzero(masks[i % 2]), o.normalize_rows(q.cpu().numpy()), 10)
        assert np.array_equal(rows.cpu().numpy(), r_ref) and np.array_equal(dist.cpu().numpy(), d_ref), i
    ix.close()


def test_a_wrong_word_count_is_einval(env):
    _, Index = env
    rng = np.random.default_rng(35)
    n, dim = 1_000, 64
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), rng.standard_normal((n, dim)).astype(np.float32))
    q = rng.standard_normal((2, dim)).astype(np.float32)
    for nwords in (31, 33, 0):
        with pytest.raises(native.NativeLibraryError, match="nwords"):
            ix.search_masked(q, np.full(nwords, 0xFFFFFFFF, dtype=np.uint32), 5)
    with pytest.raises(ValueError):
        ix.search_masked(q, np.ones(n - 1, dtype=bool), 5)
    dist, rows = ix.search_masked(q, np.full(32, 0xFFFFFFFF, dtype=np.uint32), 5)
    d0, r0 = ix.search(q, 5)
    assert np.array_equal(rows, r0) and np.array_equal(dist, d0)
    ix.close()


def test_masked_dense_passes_do_not_feed_the_filter_watch(env):
    """The index reads its pass counters back after each of its first 32 searches and after every 8th from then on; int8 passes
    that left more than "shadow8_max_surv" survivors per query start a cooldown.  34 unmasked searches bring the index to where no
    read-back is pending; then the limit is set to ONE survivor per query, and 13 masked dense searches cross the next
    read-back point (search 40) and the one where its result is looked at (41).  Had they fed the watch, a cooldown would
    have started there."""
    torch, Index = env
    rng = np.random.default_rng(36)
    n, dim, B = 40_000, 768, 140
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)                                        # (the cooldown stays at its default of 256 searches)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    for _ in range(34):
        ix.search(q, 10)
        torch.cuda.synchronize()
    assert ix.stat("searches") == 34 and ix.stat("i8v2_passes") == 34 and ix.stat("shadow8_cooldowns") == 0
    ix.set_option("shadow8_max_surv", 1)
    ix.set_option("mask_route", DENSE)
    allow = rng.random(n) < 0.5
    for _ in range(13):
        ix.search_masked(q, allow, 10)
        torch.cuda.synchronize()
    assert ix.stat("mask_dense_searches") == 13 and ix.stat("i8v2_passes") == 47
    assert ix.stat("mask_filter_survivors") > 13 * B, "the masked passes did leave more than one survivor per query"
    assert ix.stat("shadow8_cooldowns") == 0
    ix.search(q, 10)                                                 # search 48: the int8 tile filter, as before the masked passes
    assert ix.stat("i8v2_passes") == 48 and ix.stat("shadow8_cooldowns") == 0
    # ... and the watch itself works at this limit: that unmasked pass is read back and starts a cooldown at the next look
    torch.cuda.synchronize()
    ix.search(q, 10)
    assert ix.stat("shadow8_cooldowns") == 1
    ix.close()


def test_collection_query_with_a_general_where_against_the_checker_engine(env):
    rng = np.random.default_rng(37)
    n, dim = 3_000, 96
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    types = ["counter", "gauge", "histogram"]
    mds = [{"namespace": f"ns{i % 4}", "type": types[i % 3], "rank": i} for i in range(n)]
    q = rng.standard_normal((5, dim)).astype(np.float32)
    where = {"$and": [{"type": {"$in": ["counter", "histogram"]}}, {"namespace": {"$ne": "ns2"}}, {"rank": {"$gte": 100}}]}
    answers = []
    for client in (KnnClient(), KnnClient(engine_factory=lambda d: MaskedOracleEngine(d))):
        col = client.get_or_create_collection("c")
        col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=mds)
        col.delete(ids=[f"id{i}" for i in range(100, 200)])
        answers.append(col.query(query_embeddings=q, n_results=10, where=[where, None, where, {"namespace": "ns1"}, {"type": "nobody"}]))
        if not isinstance(col._engine, MaskedOracleEngine):
            assert col._engine.stat("masked_searches") == 1 and col._engine.stat("scoped_searches") == 1, "one call per distinct filter"
    assert answers[0]["ids"] == answers[1]["ids"] and answers[0]["distances"] == answers[1]["distances"]
    assert all(len(ids) == 10 for ids in answers[0]["ids"][:4]) and answers[0]["ids"][4] == []
    assert all(int(i[2:]) >= 200 and int(i[2:]) % 3 != 1 and int(i[2:]) % 4 != 2 for i in answers[0]["ids"][0])
