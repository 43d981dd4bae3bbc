"""Global row ids up to the 32-bit limit, on every search route (include/codd_knn.h, conventions: row_base + count < 0xFFFFFFFF).

Every shard-local search returns packed keys whose low word is 0xFFFFFFFF - (row_base + row).  For an index of n rows the tests use
    TOP  = 0xFFFFFFFE - n        the last legal base: its highest global row is 0xFFFFFFFD
    SIGN = 0x80000000 - n // 2   global rows on both sides of 2^31
    OVER = 0xFFFFFFFF - n        the first illegal base
The reference is the oracle's answer at base 0 (for the restricted routes: the sub-matrix references the suite already has), its row
word rewritten in numpy uint64: expected = (keys0 & 0xFFFFFFFF00000000) | (0xFFFFFFFF - (row0 + base)), empty keys left 0.  Keys are
compared bit for bit; where an entry point also writes distances and rows, the rows must be row0 + base as int64 (-1 padded) and the
distances the bits of base 0.  A CPU test first checks that the oracle's own row_base arithmetic agrees with that rewrite.

Each route is forced by the options, and confirmed by the stat, that PATHS in test_gpu_deletes.py uses, on the smallest corpus at
which the route still runs (6,001 rows: no multiple of 4, 32 or 256).  Every corpus holds an exact tie (two equal rows, the last
query equal to them) and, for batches, 40 equal rows that the first query equals: "ties -> lower row" is what a wrapped or
sign-extended row word breaks first, and 40 hits overflow a hit list capped at 16 (the fallback routes)."""

import ctypes

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests._scoped_oracle_engine import ScopedOracleEngine
from tests.test_gpu_deletes import always_filter, expected_keys, stored
from tests.test_gpu_ivf_masked import K, N, NLIST, key_table, reference, words_of

gpu = pytest.mark.gpu   # (per test: the oracle precondition below runs without a device)

LOW, HIGH = np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF00000000)
EINVAL = -22
KEY_SENTINEL, ROW_SENTINEL, DIST_SENTINEL = 0x5A5A5A5A5A5A5A5A, -7, -123.25


def top(n):
    return 0xFFFFFFFE - n


def sign(n):
    return 0x80000000 - n // 2


def over(n):
    return 0xFFFFFFFF - n


def row0_of(keys0: np.ndarray) -> np.ndarray:
    return np.where(keys0 == 0, np.int64(-1), (LOW - (keys0 & LOW)).astype(np.int64))


def shifted(keys0: np.ndarray, base: int) -> np.ndarray:
    """the keys of base 0 with the row word of `base`, in numpy uint64; empty keys stay 0"""
    keys0 = np.ascontiguousarray(keys0, dtype=np.uint64)
    rows = (LOW - (keys0 & LOW)) + np.uint64(base)
    assert (rows[keys0 != 0] <= np.uint64(0xFFFFFFFD)).all()
    return np.where(keys0 == 0, np.uint64(0), (keys0 & HIGH) | (LOW - rows))


def shifted_rows(keys0: np.ndarray, base: int) -> np.ndarray:
    r0 = row0_of(keys0)
    return np.where(r0 < 0, np.int64(-1), r0 + np.int64(base))


def assert_keys(got: np.ndarray, keys0: np.ndarray, base: int, what):
    got, want = got.view(np.uint64), shifted(keys0, base)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, j = bad[0]
        raise AssertionError((what, hex(base), f"{bad.shape[0]} keys differ, score words equal: {bool(((got ^ want) >> np.uint64(32) == 0).all())}",
                              f"first at {b, j}: got {int(got[b, j]):#018x} want {int(want[b, j]):#018x}"))


def corpus(rng, n, dim, B):
    """raw rows and queries; rows a < b are equal and the last query equals them; for B > 1, 40 more rows are equal to each other
    and to the first query"""
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    picks = rng.choice(n, size=42, replace=False)
    a, b = sorted(picks[:2].tolist())
    raw[b] = raw[a]
    q[-1] = raw[a]
    clones = np.sort(picks[2:])
    if B > 1:
        raw[clones] = raw[clones[0]]
        q[0] = raw[clones[0]]
    return raw, q, (a, b), clones


def assert_ties_lead(keys0, pair, clones, B):
    """the premise of the tie cases: the oracle's answer starts with the equal rows, lower row first, on one score word"""
    r0 = row0_of(keys0)
    assert r0[-1, :2].tolist() == list(pair) and keys0[-1, 0] >> np.uint64(32) == keys0[-1, 1] >> np.uint64(32)
    if B > 1:
        lead = min(keys0.shape[1], clones.size)
        assert np.array_equal(r0[0, :lead], clones[:lead]) and np.unique(keys0[0, :lead] >> np.uint64(32)).size == 1


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import ivf, knn_index

    return torch, knn_index, ivf


# ------------------------------------------------------------------------------------------------------------------------
# the precondition, on the CPU: the C oracle's row_base arithmetic and the numpy rewrite agree before either judges a kernel
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [("f32", 128), ("bf16", 384)])
def test_the_oracle_at_the_top_base_equals_the_shifted_keys_of_base_zero(dtype, dim):
    rng = np.random.default_rng(3100 + dim)
    n, B = 1_001, 5
    raw, q, pair, clones = corpus(rng, n, dim, B)
    rows_ref, qn = stored(raw, dtype), o.normalize_rows(q)
    for k in (10, 128):
        keys0 = o.search_keys(rows_ref, dtype, qn, k, 0)
        assert_ties_lead(keys0, pair, clones, B)
        for base in (top(n), sign(n), 1):
            assert np.array_equal(o.search_keys(rows_ref, dtype, qn, k, base), shifted(keys0, base)), (dtype, k, hex(base))
        assert shifted_rows(keys0, top(n)).max() <= 0xFFFFFFFD and shifted_rows(keys0, sign(n)).min() < 2**31 <= shifted_rows(keys0, sign(n)).max()
    few = o.search_keys(rows_ref[:3], dtype, qn, 10, 0)                      # empty keys stay empty
    assert np.array_equal(o.search_keys(rows_ref[:3], dtype, qn, 10, top(3)), shifted(few, top(3))) and (shifted(few, top(3))[:, 3:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# the unrestricted routes: codd_knn_search_keys, one search at k = 10 (scan_k128: 128) and base TOP per route; the exact
# scan and the int8 tile filter at SIGN as well
# ------------------------------------------------------------------------------------------------------------------------
ROUTES = [
    # name, dtype, dim, n, B, k, filter forced on whatever the size, options, stat that must move, also at SIGN
    ("scan_small", "f32", 128, 6_001, 8, 10, False, {}, "scan_launches", True),
    ("scan_off", "bf16", 384, 6_001, 40, 10, False, {"filter": 0}, "scan_launches", True),
    ("scan_k128", "f16", 384, 6_001, 5, 128, False, {"filter": 0}, "scan_launches", True),
    ("bf16_gemm", "f32", 128, 6_001, 40, 10, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes", False),
    ("bf16_gemm_b200", "bf16", 384, 6_001, 200, 10, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes", False),
    ("f16_tile", "f32", 384, 6_001, 200, 10, True, {"shadow8": 0}, "f16_tile_passes", False),
    ("i8_gen1", "f32", 128, 6_001, 40, 10, True, {"i8v2": 0}, "shadow8_passes", False),
    ("i8_tile_half", "f32", 384, 6_001, 100, 10, True, {}, "i8v2_passes", True),
    ("i8_tile", "f32", 384, 6_001, 256, 10, True, {}, "i8v2_passes", True),
    ("fallback", "f32", 384, 6_001, 140, 10, True, {"hit_cap": 16}, "fallback_queries", False),
    ("fallback_unfused", "f32", 384, 6_001, 40, 10, True, {"hit_cap": 16}, "fallback_queries", False),
    ("small_batch", "f32", 384, 6_001, 1, 10, True, {"small_batch_max": 1}, "small_batch_passes", False),
    ("wide_f32_1536", "f32", 1536, 6_001, 8, 10, False, {}, "scan_launches", False),
    ("wide_f32_1536_filter", "f32", 1536, 6_001, 140, 10, True, {}, "filter_passes", False),
    ("wide_bf16_4096", "bf16", 4096, 6_001, 6, 10, False, {}, "scan_launches", False),
]


@gpu
@pytest.mark.parametrize("name,dtype,dim,n,B,k,forced,options,moved,at_sign", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_writes_global_rows_up_to_the_limit(env, name, dtype, dim, n, B, k, forced, options, moved, at_sign):
    _, knn_index, _ = env
    rng = np.random.default_rng(3200 + len(name) * 1000 + dim + B)
    raw, q, pair, clones = corpus(rng, n, dim, B)
    keys0 = o.search_keys(stored(raw, dtype), dtype, o.normalize_rows(q), k, 0)
    assert_ties_lead(keys0, pair, clones, B)
    ix = knn_index.DeviceKnnIndex(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    if forced:
        always_filter(ix)
    for key, value in options.items():
        ix.set_option(key, value)
    for base in (top(n), sign(n)) if at_sign else (top(n),):
        before = ix.stat(moved)
        keys = ix.search_keys(q, k, row_base=base).cpu().numpy()
        print(f"{name}: {n} x {dim} {dtype}, B = {B}, k = {k}, base {base:#x}: {moved} {before} -> {ix.stat(moved)}")
        assert_keys(keys, keys0, base, name)
        assert ix.stat(moved) > before, (name, moved)
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# the restricted routes share one index: N rows (no multiple of 32) with scope labels and an IVF layout the test installs
# itself, so that it knows every list's rows (as test_gpu_ivf_masked.py does)
# ------------------------------------------------------------------------------------------------------------------------
class Ctx:
    pass


DIM, BMAX, NPROBE = 128, 256, 8
TIE = 1                                     # the query that equals the two equal rows (query 0 equals the 40)


@pytest.fixture(scope="module")
def ctx(env):
    torch, knn_index, _ = env
    c = Ctx()
    c.torch = torch
    rng = np.random.default_rng(3300)
    c.raw, c.queries, c.pair, c.clones = corpus(rng, N, DIM, BMAX)
    c.queries[1] = c.queries[-1]                            # the query of the equal rows is in every batch of two or more: TIE
    c.rows_ref = stored(c.raw, "f32")
    qn = o.normalize_rows(c.queries)
    cent = rng.standard_normal((NLIST, DIM)).astype(np.float32)
    _, c.probed = o.search(o.normalize_rows(cent), "f32", qn, NLIST)
    c.assign = rng.choice(np.delete(np.arange(NLIST), 3), size=N, p=np.r_[0.3, 0.2, np.full(NLIST - 3, 0.5 / (NLIST - 3))])
    c.assign[list(c.pair)] = c.probed[TIE, 0]          # the equal rows share a list that their query probes first, the 40 as well
    c.assign[c.clones] = c.probed[0, 0]
    perm = np.argsort(c.assign, kind="stable").astype(np.int64)
    offsets = np.zeros(NLIST + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(c.assign, minlength=NLIST))
    c.labels = rng.integers(0, 5, N).astype(np.uint32)
    c.labels[list(c.pair)] = 4
    c.labels[c.clones] = 1
    c.mask = rng.random(N) < 0.3
    c.mask[list(c.pair)] = True
    c.mask[c.clones] = True
    c.key_of = key_table(c.rows_ref, "f32", qn)
    c.lib = native.load()
    c.ix = knn_index.DeviceKnnIndex(DIM, dtype="f32")
    c.ix.upsert(np.arange(N, dtype=np.int64), c.raw)
    c.ix.set_scopes(np.arange(N, dtype=np.int64), c.labels)
    t = [torch.from_numpy(a).to(c.ix.device) for a in (cent, perm, offsets)]
    native.check(c.lib.codd_knn_ivf_install(c.ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), c.ix._stream()), "codd_knn_ivf_install")
    c.oracle = ScopedOracleEngine(DIM, "f32")
    c.oracle.upsert(np.arange(N, dtype=np.int64), c.raw)
    c.oracle.set_scopes(np.arange(N, dtype=np.int64), c.labels)
    yield c
    c.ix.close()


def fresh_outputs(torch, B, k):
    return (torch.full((B, k), KEY_SENTINEL, dtype=torch.int64, device="cuda:0"), torch.full((B, k), DIST_SENTINEL, dtype=torch.float32, device="cuda:0"),
            torch.full((B, k), ROW_SENTINEL, dtype=torch.int64, device="cuda:0"))


def untouched(outs):
    keys, dist, rows = outs
    return bool((keys == KEY_SENTINEL).all() and (dist == DIST_SENTINEL).all() and (rows == ROW_SENTINEL).all())


def entry_points(c, B, k=K):
    """name -> call(base, (keys, dist, rows)) -> rc: the seven entry points that take a row_base, through ctypes as they are, on the
    first B queries; everything they read is kept alive in the closure"""
    torch, lib, ix = c.torch, c.lib, c.ix
    h, st = ix._h, ix._stream()
    q = torch.from_numpy(c.queries[:B]).to(ix.device)
    scopes_np = (np.arange(B) % 6).astype(np.uint32)                # 0 .. 5; nobody carries 5
    scopes_np[TIE] = 4 if B % 2 else 0                              # the query of the equal rows: in their scope, or in scope 0
    scopes = torch.from_numpy(scopes_np.view(np.int32)).to(ix.device)
    words = words_of(c.mask)                                        # (garbage above the count in the last word)
    dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
    nw = words.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731
    calls = {
        "search_keys": lambda base, o3: lib.codd_knn_search_keys(h, p(q), B, k, base, p(o3[0]), st),
        "search_scoped": lambda base, o3: lib.codd_knn_search_scoped(h, p(q), p(scopes), B, k, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
        "search_masked": lambda base, o3: lib.codd_knn_search_masked(h, p(q), B, k, words.ctypes.data, nw, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
        "search_masked_dev": lambda base, o3: lib.codd_knn_search_masked_dev(h, p(q), B, k, p(dev_words), nw, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
        "ivf_search": lambda base, o3: lib.codd_knn_ivf_search(h, p(q), B, k, NPROBE, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
        "ivf_search_masked": lambda base, o3: lib.codd_knn_ivf_search_masked(h, p(q), B, k, NPROBE, words.ctypes.data, nw, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
        "ivf_search_masked_dev": lambda base, o3: lib.codd_knn_ivf_search_masked_dev(h, p(q), B, k, NPROBE, p(dev_words), nw, base, p(o3[0]), p(o3[1]), p(o3[2]), st),
    }
    return calls, scopes_np


def run(c, call, base, B, k=K):
    """(rc, keys u64, dist, rows) of one call with all three outputs"""
    outs = fresh_outputs(c.torch, B, k)
    rc = call(base, outs)
    c.torch.cuda.synchronize()
    return rc, outs[0].cpu().numpy().view(np.uint64), outs[1].cpu().numpy(), outs[2].cpu().numpy()


def check_entry(c, call, keys0, B, what, has_ranks=True):
    """the entry point at TOP against the shifted reference: keys bit for bit, rows = row0 + base (int64, positive, -1 padded),
    distances the bits of the same call at base 0 (which are the oracle's)"""
    base = top(N)
    rc0, k0, d0, r0 = run(c, call, 0, B)
    rc, keys, dist, rows = run(c, call, base, B)
    assert rc0 == 0 and rc == 0, (what, rc0, rc, native.last_error())
    assert_keys(k0, keys0, 0, what)
    assert_keys(keys, keys0, base, what)
    if has_ranks:
        want_rows = shifted_rows(keys0, base)
        assert rows.dtype == np.int64 and np.array_equal(rows, want_rows), (what, "rows")
        assert ((rows > 0) | (rows == -1)).all() and rows.max() <= 0xFFFFFFFD and rows.max() > 2**31
        assert np.array_equal(dist.view(np.uint32), d0.view(np.uint32)), (what, "dist changed with the base")
        assert np.array_equal(d0.view(np.uint32), o.unpack_keys(keys0)[0].view(np.uint32)) and np.array_equal(r0, row0_of(keys0)), (what, "base 0")


@gpu
def test_scoped_search_with_scope_zero_and_real_scopes_in_one_batch(ctx):
    c = ctx
    for B in (64, 9):
        calls, scopes = entry_points(c, B)
        keys0 = c.oracle.search_keys_scoped(c.queries[:B], scopes, K, 0)
        assert row0_of(keys0)[TIE, :2].tolist() == list(c.pair) and (keys0[scopes == 5] == 0).all() and (keys0[scopes != 5] != 0).all()
        before = c.ix.stat("scoped_searches")
        check_entry(c, calls["search_scoped"], keys0, B, ("scoped", B))
        assert c.ix.stat("scoped_searches") == before + 2


@gpu
@pytest.mark.parametrize("route,stat", [(1, "mask_list_searches"), (2, "mask_dense_searches")], ids=["list", "dense"])
def test_masked_search_host_words_and_device_words(ctx, route, stat):
    c = ctx
    c.ix.set_option("mask_route", route)
    try:
        for B in (9, 140):
            calls, _ = entry_points(c, B)
            keys0 = expected_keys(c.rows_ref, "f32", c.mask, c.queries[:B], K, 0)
            assert row0_of(keys0)[TIE, :2].tolist() == list(c.pair) and np.array_equal(row0_of(keys0)[0], c.clones[:K])
            for name in ("search_masked", "search_masked_dev"):
                before = {key: c.ix.stat(key) for key in (stat, "masked_searches", "masked_dev_searches")}
                check_entry(c, calls[name], keys0, B, (name, route, B))
                assert c.ix.stat(stat) == before[stat] + 2 and c.ix.stat("masked_searches") == before["masked_searches"] + 2
                assert c.ix.stat("masked_dev_searches") == before["masked_dev_searches"] + (2 if name.endswith("dev") else 0)
    finally:
        c.ix.set_option("mask_route", 0)


@gpu
@pytest.mark.parametrize("share,B", [(0, 9), (1, BMAX)], ids=["per_pair", "shared"])
def test_ivf_search_plain_and_masked(ctx, share, B):
    """B * NPROBE = 72 (query, list) pairs go list by list per pair; 2,048 pairs (>= 1,024 and >= 2 * NLIST) share the lists' scans"""
    c = ctx
    c.ix.set_option("ivf_share", share)
    try:
        calls, _ = entry_points(c, B)
        none_dead = np.zeros(N, dtype=bool)
        for name, mask in (("ivf_search", np.ones(N, dtype=bool)), ("ivf_search_masked", c.mask), ("ivf_search_masked_dev", c.mask)):
            keys0 = reference(c, B, NPROBE, mask, none_dead)
            assert row0_of(keys0)[TIE, :2].tolist() == list(c.pair) and np.array_equal(row0_of(keys0)[0], c.clones[:K])
            before = {key: c.ix.stat(key) for key in ("ivf_shared_searches", "ivf_masked_searches")}
            check_entry(c, calls[name], keys0, B, (name, share, B))
            assert c.ix.stat("ivf_shared_searches") == before["ivf_shared_searches"] + 2 * share, (name, share)
            assert c.ix.stat("ivf_masked_searches") == before["ivf_masked_searches"] + (2 if "masked" in name else 0)
    finally:
        c.ix.set_option("ivf_share", 1)


# ------------------------------------------------------------------------------------------------------------------------
# the error contract: at OVER every entry point refuses, says why, writes nothing and counts nothing; at TOP it answers
# ------------------------------------------------------------------------------------------------------------------------
COUNTERS = ("searches", "scan_launches", "ivf_masked_searches", "masked_searches", "scoped_searches")
ENTRY_POINTS = ("search_keys", "search_scoped", "search_masked", "search_masked_dev", "ivf_search", "ivf_search_masked", "ivf_search_masked_dev")


@gpu
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_first_illegal_base_is_einval_and_touches_nothing(ctx, name):
    c = ctx
    B = 9
    calls, _ = entry_points(c, B)
    assert sorted(calls) == sorted(ENTRY_POINTS)
    before = {key: c.ix.stat(key) for key in COUNTERS}
    for base in (over(N), 0xFFFFFFFF):
        outs = fresh_outputs(c.torch, B, K)
        rc = calls[name](base, outs)
        message = native.last_error()
        c.torch.cuda.synchronize()
        assert rc == EINVAL, (name, hex(base), rc)
        assert "32 bits" in message, (name, message)
        assert untouched(outs), (name, hex(base), "outputs written")
        assert {key: c.ix.stat(key) for key in COUNTERS} == before, (name, hex(base))
    outs = fresh_outputs(c.torch, B, K)
    assert calls[name](top(N), outs) == 0, (name, native.last_error())
    c.torch.cuda.synchronize()
    assert not (outs[0] == KEY_SENTINEL).any() and (name == "search_keys" or not (outs[2] == ROW_SENTINEL).any())


@gpu
def test_the_python_wrappers_refuse_what_ctypes_would_truncate(ctx, env):
    _, _, ivf = env
    c, ix, q = ctx, ctx.ix, ctx.queries[:3]
    scopes = np.zeros(3, dtype=np.uint32)
    dev_words = c.torch.from_numpy(words_of(c.mask).view(np.int32)).to(ix.device)
    wrappers = {
        "search_keys": lambda b: ix.search_keys(q, K, b),
        "search_keys_scoped": lambda b: ix.search_keys_scoped(q, scopes, K, b),
        "search_keys_masked": lambda b: ix.search_keys_masked(q, c.mask, K, b),
        "search_keys_masked_dev": lambda b: ix.search_keys_masked_dev(q, dev_words, K, b),
        "ivf_search_masked_tensors": lambda b: ix.ivf_search_masked_tensors(q, c.mask, K, NPROBE, b),
        "ivf_search_keys_masked": lambda b: ix.ivf_search_keys_masked(q, c.mask, K, NPROBE, b),
        "ivf_search_masked_dev_tensors": lambda b: ix.ivf_search_masked_dev_tensors(q, dev_words, K, NPROBE, b),
        "ivf_search_keys_masked_dev": lambda b: ix.ivf_search_keys_masked_dev(q, dev_words, K, NPROBE, b),
        "search_ivf": lambda b: ivf.search_ivf(ix, q, K, NPROBE, b),
        "search_ivf_keys": lambda b: ivf.search_ivf_keys(ix, q, K, NPROBE, b),
        "search_ivf allow": lambda b: ivf.search_ivf(ix, q, K, NPROBE, b, allow=c.mask),
        "search_ivf_keys allow": lambda b: ivf.search_ivf_keys(ix, q, K, NPROBE, b, allow=dev_words),
    }
    before = {key: ix.stat(key) for key in COUNTERS}
    for name, call in wrappers.items():
        for bad in (over(N), -1, 2**32, 2**32 + 5):
            with pytest.raises(ValueError, match="32 bits"):
                call(bad)
    assert {key: ix.stat(key) for key in COUNTERS} == before, "a refused base never reaches the library"
    want = shifted(o.search_keys(c.rows_ref, "f32", o.normalize_rows(q), K, 0), top(N))
    assert np.array_equal(wrappers["search_keys"](top(N)).cpu().numpy().view(np.uint64), want)
    assert np.array_equal(wrappers["search_ivf_keys"](top(N)).cpu().numpy().view(np.uint64), shifted(reference(c, 3, NPROBE, np.ones(N, dtype=bool), np.zeros(N, dtype=bool)), top(N)))


# ------------------------------------------------------------------------------------------------------------------------
# composition: two shards of one corpus at the very top of the range, merged; then under one mask over 0xFFFFFFFE global rows
# ------------------------------------------------------------------------------------------------------------------------
GLOBAL_ROWS = 0xFFFFFFFE
GLOBAL_WORDS = 1 << 27                      # ceil(0xFFFFFFFE / 32): 512 MiB of int32


@pytest.fixture(scope="module")
def shards(env):
    torch, knn_index, _ = env
    c = Ctx()
    c.n, c.dim, c.cut = 6_011, 128, 2_605                              # 2,605 = 81 * 32 + 13
    rng = np.random.default_rng(3400)
    c.raw, c.q, c.pair, c.clones = corpus(rng, c.n, c.dim, 7)
    c.raw[c.cut + 9] = c.raw[40]                                       # one more exact tie, across the cut
    c.q[3] = c.raw[40]
    c.rows_ref = stored(c.raw, "f32")
    c.n1, c.n2 = c.cut, c.n - c.cut
    c.bases = (top(c.n2) - c.n1, top(c.n2))                            # shard 2 at its last legal base, shard 1 just below it
    assert c.bases[0] == GLOBAL_ROWS - c.n
    c.mask = rng.random(c.n) < 0.3
    c.mask[[40, c.cut + 9, *c.pair]] = True
    c.mask[c.clones[::2]] = True
    c.ix = []
    for lo, hi in ((0, c.cut), (c.cut, c.n)):
        s = knn_index.DeviceKnnIndex(c.dim)
        s.upsert(np.arange(hi - lo, dtype=np.int64), c.raw[lo:hi])
        c.ix.append(s)
    # the global mask, allocated once: zeros, then garbage below the first shard, the mask over the two shards, and garbage in the
    # two bits of the last word that lie at and above global_rows
    c.first_word = (c.bases[0] >> 5) - 2
    c.first_row = c.first_word * 32
    region = np.zeros((GLOBAL_WORDS - c.first_word) * 32, dtype=bool)
    region[: c.bases[0] - c.first_row] = rng.random(c.bases[0] - c.first_row) < 0.5
    region[c.bases[0] - c.first_row : GLOBAL_ROWS - c.first_row] = c.mask
    c.region = region[: GLOBAL_ROWS - c.first_row].copy()             # what numpy slices: the bits of real global rows
    region[GLOBAL_ROWS - c.first_row :] = True
    c.global_words = torch.zeros(GLOBAL_WORDS, dtype=torch.int32, device="cuda:0")
    c.global_words[c.first_word :] = torch.from_numpy(np.packbits(region, bitorder="little").view("<u4").view(np.int32).copy()).to("cuda:0")
    yield c
    for s in c.ix:
        s.close()
    del c.global_words


def merged_both_ways(knn_index, torch, parts, k):
    """(keys u64, dist, rows) through merge_keys on [B, 2k] and through merge_shards on the all_gather layout: they must agree"""
    a = knn_index.merge_keys(torch.cat(parts, dim=1).contiguous(), k)
    b = knn_index.merge_shards(torch.cat(parts, dim=0).contiguous(), 2, k)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    return a[0].cpu().numpy().view(np.uint64), a[1].cpu().numpy(), a[2].cpu().numpy()


def assert_merged(got, keys0, base, what):
    keys, dist, rows = got
    assert_keys(keys, keys0, base, what)
    assert rows.dtype == np.int64 and np.array_equal(rows, shifted_rows(keys0, base)), (what, "rows")
    assert np.array_equal(dist.view(np.uint32), o.unpack_keys(keys0)[0].view(np.uint32)), (what, "dist")


@gpu
def test_two_shards_at_the_top_of_the_range_merge_to_the_whole_corpus(env, shards):
    torch, knn_index, _ = env
    c, k = shards, 10
    keys0 = o.search_keys(c.rows_ref, "f32", o.normalize_rows(c.q), k, 0)
    assert row0_of(keys0)[3, :2].tolist() == [40, c.cut + 9] and row0_of(keys0)[-1, :2].tolist() == list(c.pair)
    parts = [s.search_keys(c.q, k, row_base=b) for s, b in zip(c.ix, c.bases)]
    assert_merged(merged_both_ways(knn_index, torch, parts, k), keys0, c.bases[0], "two shards")


def numpy_slice(c, row_base, count):
    local = np.zeros(count, dtype=bool)
    have = c.region[row_base - c.first_row : row_base - c.first_row + count]
    local[: have.shape[0]] = have
    return words_of(local, garbage_above=False)


@gpu
def test_two_shards_under_one_mask_over_all_32_bit_global_rows(env, shards):
    torch, knn_index, _ = env
    c, k = shards, 10
    for row_base, count in ((c.bases[0], c.n1), (c.bases[1], c.n2), (c.bases[1], c.n2 + 40), (c.bases[0] - 37, 100), (GLOBAL_ROWS - 1, 33), (GLOBAL_ROWS, 5)):
        got = knn_index.slice_mask(c.global_words, GLOBAL_ROWS, row_base, count).cpu().numpy().view(np.uint32)
        want = numpy_slice(c, row_base, count)
        assert got.shape == want.shape and np.array_equal(got, want), (hex(row_base), count, np.flatnonzero(got != want)[:8])
    assert np.array_equal(numpy_slice(c, c.bases[0], c.n1), words_of(c.mask[: c.cut], garbage_above=False))
    keys0 = expected_keys(c.rows_ref, "f32", c.mask, c.q, k, 0)
    assert row0_of(keys0)[3, :2].tolist() == [40, c.cut + 9] and row0_of(keys0)[-1, :2].tolist() == list(c.pair)
    parts = []
    for s, base in zip(c.ix, c.bases):
        local = s.slice_mask(c.global_words, GLOBAL_ROWS, base)
        before = s.stat("masked_dev_searches")
        parts.append(s.search_keys_masked_dev(c.q, local, k, base))
        assert s.stat("masked_dev_searches") == before + 1
    assert_merged(merged_both_ways(knn_index, torch, parts, k), keys0, c.bases[0], "two shards, one global mask")
