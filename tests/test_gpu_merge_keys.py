"""codd_knn_merge_keys / codd_knn_merge_shards entered directly, against plain numpy (every search route ends in merge_keys_kernel:
WaveTopK::offer_lanes over the input, merge_lists over the four waves, write_ranks).

The reference of the keys is `np.sort(keys, axis=1)[:, ::-1][:, :k]`, zero padded when m < k; of the decoded outputs
`rows = where(key == 0, -1, 0xFFFFFFFF - low)` and `dist = where(key == 0, inf, float32(1) - unord(high))` in float32.  All three are
compared bit for bit.  The keys are packed in numpy from (score, row) pairs the way make_key packs them (wave_topk.h), so only keys
a search can produce go in: scores from a pool of extremes (both infinities, both zeros, denormals, the neighbours of 1, values far
outside (-1, 1)) plus random normals, rows from 0, 1, 2^31 - 1, 2^31, 0xFFFFFFFD plus random ones."""

import ctypes

import numpy as np
import pytest

gpu = pytest.mark.gpu   # (per test: the check of the numpy packing itself runs without a device)

LOW = np.uint64(0xFFFFFFFF)
EINVAL = -22
SCORE_POOL = np.array([-np.inf, -3.5, -1.0, -1e-40, -0.0, 0.0, 1e-40, 0.25, 1.0 - 2.0**-24, 1.0, 1.0 + 2.0**-23, 3e38, np.inf], dtype=np.float32)
ROW_POOL = np.array([0, 1, 2**31 - 1, 2**31, 0xFFFFFFFD], dtype=np.uint64)
KEY_SENTINEL, ROW_SENTINEL, DIST_SENTINEL = 0x5A5A5A5A5A5A5A5A, -7, -123.25


# ---- the documented packing, in numpy -------------------------------------------------------------------------------------------
def ord_f32(scores: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unord_f32(o: np.ndarray) -> np.ndarray:
    o = o.astype(np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def make_keys(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    return (ord_f32(scores).astype(np.uint64) << np.uint64(32)) | (LOW - rows.astype(np.uint64))


def random_keys(rng, shape, empty_share=0.0) -> np.ndarray:
    """keys of random (score, row) pairs: a third of the scores and a quarter of the rows from the pools of extremes"""
    size = int(np.prod(shape))
    scores = rng.standard_normal(size).astype(np.float32)
    pick = rng.random(size) < 1 / 3
    scores[pick] = rng.choice(SCORE_POOL, size=int(pick.sum()))
    rows = rng.integers(0, 0xFFFFFFFE, size=size, dtype=np.uint64)
    pick = rng.random(size) < 1 / 4
    rows[pick] = rng.choice(ROW_POOL, size=int(pick.sum()))
    keys = make_keys(scores, rows)
    assert (keys != 0).all()
    if empty_share:
        keys[rng.random(size) < empty_share] = 0
    return keys.reshape(shape)


def distinct_keys(rng, count) -> np.ndarray:
    keys = np.unique(random_keys(rng, (2 * count + 64,)))
    return rng.permutation(keys)[:count]


def pool_product() -> np.ndarray:
    """every pool score with every pool row"""
    return make_keys(np.repeat(SCORE_POOL, ROW_POOL.size), np.tile(ROW_POOL, SCORE_POOL.size))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def top_k(keys: np.ndarray, k: int) -> np.ndarray:
    B, m = keys.shape
    out = np.zeros((B, k), dtype=np.uint64)
    best = np.sort(keys, axis=1)[:, ::-1][:, :k]
    out[:, : best.shape[1]] = best
    return out


def decode(keys: np.ndarray):
    rows = np.where(keys == 0, np.int64(-1), (LOW - (keys & LOW)).astype(np.int64))
    with np.errstate(invalid="ignore"):
        dist = np.where(keys == 0, np.float32(np.inf), np.float32(1) - unord_f32(keys >> np.uint64(32))).astype(np.float32)
    return dist, rows


# ---- the two entry points through ctypes, outputs pre-filled with sentinels, any of them NULL -----------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import knn_index, native

    return torch, native.load(), knn_index


def outputs(torch, B, k, want):
    B, k = max(B, 1), min(max(k, 1), 256)
    keys = torch.full((B, k), KEY_SENTINEL, dtype=torch.int64, device="cuda:0") if want[0] else None
    dist = torch.full((B, k), DIST_SENTINEL, dtype=torch.float32, device="cuda:0") if want[1] else None
    rows = torch.full((B, k), ROW_SENTINEL, dtype=torch.int64, device="cuda:0") if want[2] else None
    return keys, dist, rows


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host(t):
    return None if t is None else t.cpu().numpy()


def stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_merge_keys(env, keys: np.ndarray, k: int, want=(True, True, True)):
    torch, lib, _ = env
    B, m = keys.shape
    src = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    out = outputs(torch, B, k, want)
    rc = lib.codd_knn_merge_keys(0, ptr(src), B, m, k, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream(torch))
    torch.cuda.synchronize()
    return rc, tuple(host(t) for t in out)


def call_merge_shards(env, flat: np.ndarray, G: int, B: int, k_in: int, k: int, want=(True, True, True)):
    torch, lib, _ = env
    src = torch.from_numpy(flat.view(np.int64)).to("cuda:0")
    out = outputs(torch, B, k, want)
    rc = lib.codd_knn_merge_shards(0, ptr(src), G, B, k_in, k, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream(torch))
    torch.cuda.synchronize()
    return rc, tuple(host(t) for t in out)


def assert_outputs(got, want_keys: np.ndarray, what):
    keys, dist, rows = got
    d_ref, r_ref = decode(want_keys)
    if keys is not None:
        bad = np.flatnonzero((keys.view(np.uint64) != want_keys).any(axis=1))
        assert bad.size == 0, (what, "keys", bad[:4], keys.view(np.uint64)[bad[:1]], want_keys[bad[:1]])
    if rows is not None:
        assert rows.dtype == np.int64 and np.array_equal(rows, r_ref), (what, "rows")
    if dist is not None:
        assert dist.dtype == np.float32 and np.array_equal(dist.view(np.uint32), d_ref.view(np.uint32)), (what, "dist")


def check_merge_keys(env, keys: np.ndarray, k: int, what):
    rc, got = call_merge_keys(env, keys, k)
    assert rc == 0, (what, rc)
    assert_outputs(got, top_k(keys, k), what)


# ---- the reference's own parts, on the CPU --------------------------------------------------------------------------------------
def test_the_numpy_packing_orders_keys_like_the_pairs_and_decodes_back():
    """(no GPU) a higher score gives a larger key, among equal scores the lower row does; unord inverts ord bit for bit"""
    assert (np.diff(ord_f32(SCORE_POOL).astype(np.int64)) > 0).all()          # (the pool is written in ascending order, -0.0 below +0.0)
    assert np.array_equal(unord_f32(ord_f32(SCORE_POOL)).view(np.uint32), SCORE_POOL.view(np.uint32))
    keys = make_keys(np.full(ROW_POOL.size, 0.25, dtype=np.float32), ROW_POOL)
    assert (keys[:-1] > keys[1:]).all() and (keys != 0).all()
    dist, rows = decode(np.array([[0, make_keys(np.float32([1.0]), np.uint64([2**31]))[0]]], dtype=np.uint64))
    assert rows.tolist() == [[-1, 2**31]] and np.isinf(dist[0, 0]) and dist[0, 1] == 0.0


# ---- merge_keys: shapes -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1000, 4096, 100_003])
def test_merge_keys_shapes(env, m):
    rng = np.random.default_rng(4000 + m)
    keys = random_keys(rng, (3, m), empty_share=0.05 if m > 1 else 0.0)
    pool = pool_product()
    keys[0, : min(m, pool.size)] = rng.permutation(pool)[: min(m, pool.size)]     # every extreme meets every extreme row in one list
    for k in (1, 63, 64, 65, 127, 128):
        check_merge_keys(env, keys, k, (m, k))


@gpu
def test_merge_keys_full_batch(env):
    rng = np.random.default_rng(4100)
    check_merge_keys(env, random_keys(rng, (1024, 257), empty_share=0.05), 65, "B = 1024")


# ---- merge_keys: arrival orders -----------------------------------------------------------------------------------------------------
def arrival_orders(rng, m, k):
    pool = distinct_keys(rng, m)
    asc = np.sort(pool)
    one = np.zeros(m, dtype=np.uint64)
    one[rng.integers(m)] = pool[0]
    thrice = np.zeros(m, dtype=np.uint64)
    thrice[: m // 3 * 3] = np.repeat(pool[: m // 3], 3)
    few = np.zeros(m, dtype=np.uint64)
    few[: k - 1] = rng.permutation(pool[: k - 1])
    # the k best keys at the very end of the list: the last 64 positions (the last step of a wave) hold the 64 best of them, in
    # random order, the rest of the k best (k > 64) the positions just before; everything in front is worse
    tail = asc.copy()
    tail[: m - k] = rng.permutation(asc[: m - k])
    tail[m - k : m - min(k, 64)] = rng.permutation(asc[m - k : m - min(k, 64)])
    tail[m - min(k, 64) :] = rng.permutation(asc[m - min(k, 64) :])
    return {
        "ascending": asc,                                  # every candidate displaces the threshold
        "descending": asc[::-1].copy(),
        "random": pool,
        "all equal": np.full(m, pool[0], dtype=np.uint64),
        "one among zeros": one,
        "three times each": rng.permutation(thrice),
        "k - 1 then zeros": few,
        "best at the end": tail,
    }


@gpu
@pytest.mark.parametrize("k", [10, 65, 128])
def test_merge_keys_arrival_orders(env, k):
    rng = np.random.default_rng(4200 + k)
    m = 1000
    orders = arrival_orders(rng, m, k)
    assert len(orders) == 8
    best = np.sort(orders["random"])[::-1][:k]
    assert np.array_equal(np.sort(orders["best at the end"][m - k :])[::-1], best) and \
        np.array_equal(np.sort(orders["best at the end"][m - 64 :])[::-1][: min(k, 64)], best[: min(k, 64)])
    for name, one in orders.items():
        keys = np.stack([one, one[::-1], np.roll(one, 37)])   # (the same multiset three ways: the answers must agree as well)
        check_merge_keys(env, keys, k, (name, k))


# ---- merge_shards -------------------------------------------------------------------------------------------------------------------
def shard_lists(rng, G, B, k_in, descending=True):
    """[G, B, k_in]: each shard's list for a query, descending with a zero tail of random length (as a shard search returns it)"""
    lists = random_keys(rng, (G, B, k_in))
    if descending:
        lists = np.sort(lists, axis=2)[:, :, ::-1].copy()
    filled = rng.integers(0, k_in + 1, size=(G, B))
    filled[0, 0] = k_in
    lists[np.arange(k_in)[None, None, :] >= filled[:, :, None]] = 0
    return lists


def check_merge_shards(env, lists, k, what):
    _, _, knn_index = env
    torch = env[0]
    G, B, k_in = lists.shape
    flat = np.ascontiguousarray(lists).reshape(-1)          # [(g * B + q) * k_in + j]: what an all_gather delivers
    regrouped = np.ascontiguousarray(lists.transpose(1, 0, 2).reshape(B, G * k_in))
    want = top_k(regrouped, k)
    rc, got = call_merge_shards(env, flat, G, B, k_in, k)
    assert rc == 0, (what, rc)
    assert_outputs(got, want, what)
    rc, again = call_merge_keys(env, regrouped, k)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(got, again)), (what, "merge_keys on the regrouped tensor")
    return flat, got


@gpu
@pytest.mark.parametrize("G", [1, 2, 3, 8, 64])
def test_merge_shards_shapes(env, G):
    rng = np.random.default_rng(4300 + G)
    below = equal = above = 0
    for k_in in (1, 10, 100, 128):
        for k in (1, 10, 128):
            for B in (1, 9):
                check_merge_shards(env, shard_lists(rng, G, B, k_in), k, (G, k_in, k, B))
            below, equal, above = below + (k < G * k_in), equal + (k == G * k_in), above + (k > G * k_in)
    assert below and above and (equal or G != 1)   # k below and above G * k_in at every G, k == G * k_in at G = 1


@gpu
def test_merge_shards_full_batch_unsorted_lists_and_the_wrappers(env):
    torch, _, knn_index = env
    rng = np.random.default_rng(4400)
    check_merge_shards(env, shard_lists(rng, 8, 1024, 10), 10, "B = 1024")
    check_merge_shards(env, shard_lists(rng, 3, 9, 100, descending=False), 128, "unsorted")
    # the Python wrappers hand the same buffers over
    lists = shard_lists(rng, 8, 9, 10)
    flat, got = check_merge_shards(env, lists, 10, "wrappers")
    gathered = torch.from_numpy(flat.view(np.int64)).to("cuda:0").view(8 * 9, 10)
    for out in (knn_index.merge_shards(gathered, 8, 10),
                knn_index.merge_keys(gathered.view(8, 9, 10).permute(1, 0, 2).reshape(9, 80).contiguous(), 10)):
        assert all(np.array_equal(t.cpu().numpy(), g) for t, g in zip(out, got))


# ---- NULL outputs and bad arguments -------------------------------------------------------------------------------------------------
@gpu
def test_any_subset_of_the_outputs_may_be_null(env):
    rng = np.random.default_rng(4500)
    keys = random_keys(rng, (5, 300), empty_share=0.05)
    lists = shard_lists(rng, 3, 5, 100)
    for k in (10, 128):
        rc, full = call_merge_keys(env, keys, k)
        rc_s, full_s = call_merge_shards(env, lists.reshape(-1), 3, 5, 100, k)
        assert rc == 0 and rc_s == 0
        assert_outputs(full, top_k(keys, k), "full")
        for bits in range(8):
            want = tuple(bool(bits >> i & 1) for i in range(3))
            for (rc, got), ref in ((call_merge_keys(env, keys, k, want), full), (call_merge_shards(env, lists.reshape(-1), 3, 5, 100, k, want), full_s)):
                assert rc == 0, (want, rc)
                for g, f, w in zip(got, ref, want):
                    assert (g is None) == (not w) and (g is None or np.array_equal(g, f)), want


def untouched(got):
    keys, dist, rows = got
    return (keys == KEY_SENTINEL).all() and (dist == np.float32(DIST_SENTINEL)).all() and (rows == ROW_SENTINEL).all()


@gpu
def test_bad_arguments_are_einval_and_write_nothing(env):
    torch, lib, _ = env
    rng = np.random.default_rng(4600)
    src = torch.from_numpy(random_keys(rng, (4, 40)).view(np.int64)).to("cuda:0")

    def merge_keys(src_ptr, B, m, k):
        out = outputs(torch, 4, 128, (True, True, True))
        rc = lib.codd_knn_merge_keys(0, src_ptr, B, m, k, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream(torch))
        torch.cuda.synchronize()
        return rc, tuple(host(t) for t in out)

    def merge_shards(src_ptr, G, B, k_in, k):
        out = outputs(torch, 4, 128, (True, True, True))
        rc = lib.codd_knn_merge_shards(0, src_ptr, G, B, k_in, k, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream(torch))
        torch.cuda.synchronize()
        return rc, tuple(host(t) for t in out)

    good = ptr(src)
    for args in ((good, 4, 0, 10), (good, 4, -1, 10), (good, 4, 40, 0), (good, 4, 40, -3), (good, 4, 40, 129), (good, 0, 40, 10), (good, -1, 40, 10),
                 (None, 4, 40, 10)):
        rc, got = merge_keys(*args)
        assert rc == EINVAL and untouched(got), ("merge_keys", args[1:])
    for args in ((good, 0, 2, 10, 10), (good, -1, 2, 10, 10), (good, 2, 0, 10, 10), (good, 2, 2, 0, 10), (good, 2, 2, 10, 0), (good, 2, 2, 10, 129),
                 (None, 2, 2, 10, 10)):
        rc, got = merge_shards(*args)
        assert rc == EINVAL and untouched(got), ("merge_shards", args[1:])
    rc, got = merge_keys(good, 4, 40, 128)                       # ... and the same buffers with good arguments are written
    assert rc == 0 and not untouched(got)
