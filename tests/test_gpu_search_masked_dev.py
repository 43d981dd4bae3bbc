"""codd_knn_search_masked_dev on the GPU: the same mask as host words through codd_knn_search_masked and as device
words through codd_knn_search_masked_dev must give identical packed keys — on both routes, forced by "mask_route", for B = 1, 5 and
64, with tombstones, with m < k and with m == 0 — an all-ones mask the bits of codd_knn_search, and the stats count the routes.
The host-mask entry point is itself checked against the oracle in test_gpu_masked_search.py; here one case per route is, too."""

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests._deleting_oracle_engine import live_reference
from tests.test_gpu_deletes import stored

pytestmark = pytest.mark.gpu

LIST, DENSE = 1, 2
DIM, N, K = 128, 20_011, 10          # 20,011: no multiple of 32, several 256-word blocks of mask words


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    rng = np.random.default_rng(16)
    raw = rng.standard_normal((N, DIM)).astype(np.float32)
    ix = DeviceKnnIndex(DIM)
    ix.upsert(np.arange(N, dtype=np.int64), raw)
    queries = rng.standard_normal((64, DIM)).astype(np.float32)
    yield torch, ix, raw, queries
    ix.close()


def words_of(mask: np.ndarray, garbage_above: bool = False) -> np.ndarray:
    n = mask.shape[0]
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    words = words.view("<u4").copy()
    if garbage_above and n % 32:
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)   # bits at or above the count are to be ignored
    return words


def both(torch, ix, q, mask, k, route, dead=None):
    """keys of the host-mask and of the device-mask entry point on `route`; asserts they are identical and the stats moved alike"""
    ix.set_option("mask_route", route)
    words = words_of(mask, garbage_above=True)
    host = ix.search_keys_masked(q, words, k).cpu().numpy()
    s0 = {key: ix.stat(key) for key in ("masked_searches", "masked_dev_searches", "mask_list_searches", "mask_dense_searches")}
    dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
    dev = ix.search_keys_masked_dev(q, dev_words, k).cpu().numpy()
    assert np.array_equal(host, dev), (q.shape, k, route, np.flatnonzero((host != dev).any(axis=1))[:8])
    visible = mask if dead is None else mask & ~dead
    m = int(visible.sum())
    assert ix.stat("last_mask_rows") == m
    assert ix.stat("masked_searches") == s0["masked_searches"] + 1 and ix.stat("masked_dev_searches") == s0["masked_dev_searches"] + 1
    moved = (ix.stat("mask_list_searches") - s0["mask_list_searches"], ix.stat("mask_dense_searches") - s0["mask_dense_searches"])
    assert moved == ((0, 0) if m == 0 else (int(route == LIST), int(route == DENSE))), (moved, m, route)
    assert np.array_equal(dev_words.cpu().numpy(), words.view(np.int32)), "the caller's words are left as they were"
    return dev


@pytest.mark.parametrize("route", [LIST, DENSE], ids=["list", "dense"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_host_words_and_device_words_give_identical_keys(env, route, B):
    torch, ix, raw, queries = env
    rng = np.random.default_rng(B * 10 + route)
    for share in (0.003, 0.4):
        mask = rng.random(N) < share
        keys = both(torch, ix, queries[:B], mask, K, route)
        assert (keys != 0).all()
    # ... and against the oracle, through the distances / rows outputs of the device-mask entry point
    d_ref, r_ref = live_reference(stored(raw, "f32"), "f32", np.flatnonzero(mask), o.normalize_rows(queries[:B]), K)
    dist, rows = ix.search_masked_dev(queries[:B], torch.from_numpy(words_of(mask).view(np.int32)).to(ix.device), K)
    assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref)


@pytest.mark.parametrize("route", [LIST, DENSE], ids=["list", "dense"])
def test_fewer_visible_rows_than_k_and_none_at_all(env, route):
    torch, ix, _, queries = env
    mask = np.zeros(N, dtype=bool)
    mask[[3, 9_999, N - 1]] = True
    keys = both(torch, ix, queries[:5], mask, K, route)
    assert ((keys != 0).sum(axis=1) == 3).all()                # min(k, m) hits
    keys = both(torch, ix, queries[:5], np.zeros(N, dtype=bool), K, route)
    assert (keys == 0).all()                                   # m == 0: all empty, no route taken (checked in both())


def test_an_all_ones_mask_gives_the_bits_of_the_plain_search(env):
    torch, ix, _, queries = env
    ones = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=ix.device)
    plain_d, plain_r = ix.search(queries[:5], K)
    plain_keys = ix.search_keys(queries[:5], K).cpu().numpy()
    for route in (LIST, DENSE, 0):
        ix.set_option("mask_route", route)
        dist, rows = ix.search_masked_dev(queries[:5], ones, K)
        assert np.array_equal(rows, plain_r) and np.array_equal(dist, plain_d), route
        assert np.array_equal(ix.search_keys_masked_dev(queries[:5], ones, K).cpu().numpy(), plain_keys), route
        assert ix.stat("last_mask_rows") == N


def test_the_words_are_read_on_the_stream_behind_what_wrote_them(env):
    """The mask is produced by torch ops enqueued just before the call, on the same stream, and never synchronised by the caller."""
    torch, ix, raw, queries = env
    ix.set_option("mask_route", 0)
    a = np.random.default_rng(7).random(N) < 0.5
    b = np.random.default_rng(8).random(N) < 0.5
    wa = torch.from_numpy(words_of(a).view(np.int32)).to(ix.device)
    wb = torch.from_numpy(words_of(b).view(np.int32)).to(ix.device)
    dist, rows = ix.search_masked_dev(queries[:5], wa & ~wb, K)
    d_ref, r_ref = live_reference(stored(raw, "f32"), "f32", np.flatnonzero(a & ~b), o.normalize_rows(queries[:5]), K)
    assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref)


def test_bad_arguments_are_einval(env):
    from codd_query_engine_amd import native

    torch, ix, _, queries = env
    short = torch.zeros(((N + 31) // 32 - 1,), dtype=torch.int32, device=ix.device)
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.search_masked_dev(queries[:1], short, K)
    with pytest.raises(ValueError):
        ix.search_masked_dev(queries[:1], np.zeros((N + 31) // 32, dtype=np.uint32), K)   # host words belong to search_masked


def test_with_tombstones(env):
    """Last in this file: it deletes from the shared index.  Both routes, the three batch sizes; a deleted row that is allowed is
    not returned and not counted."""
    torch, ix, raw, queries = env
    rng = np.random.default_rng(99)
    dead = np.zeros(N, dtype=bool)
    dead[rng.choice(N, size=N // 10, replace=False)] = True
    ix.delete(np.flatnonzero(dead))
    rows_ref = stored(raw, "f32")
    for route in (LIST, DENSE):
        for B in (1, 5, 64):
            mask = rng.random(N) < 0.3
            mask[np.flatnonzero(dead)[:50]] = True
            both(torch, ix, queries[:B], mask, K, route, dead=dead)
            ix.set_option("mask_route", route)
            dist, rows = ix.search_masked_dev(queries[:B], torch.from_numpy(words_of(mask).view(np.int32)).to(ix.device), K)
            d_ref, r_ref = live_reference(rows_ref, "f32", np.flatnonzero(mask & ~dead), o.normalize_rows(queries[:B]), K)
            assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref), (route, B)
    ones = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=ix.device)
    plain_d, plain_r = ix.search(queries[:5], K)
    dist, rows = ix.search_masked_dev(queries[:5], ones, K)
    assert np.array_equal(rows, plain_r) and np.array_equal(dist, plain_d)
    assert ix.stat("last_mask_rows") == N - int(dead.sum())
