"""codd_knn_ivf_search_masked / _masked_dev on the GPU: a row mask under an installed IVF layout.

The test installs a layout it made itself (random centroids, every row assigned to a list by the test), so it knows every list's
rows.  Per row form the oracle scores every (query, row) pair ONCE; a reference answer is then a selection from that table: the k
best keys among the rows that are allowed, live and in the lists the oracle's exact centroid top-nprobe names.  Everything is
compared as packed keys, bit for bit; every masked search runs through the host form and the device form, which must agree."""

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests.test_gpu_deletes import stored

pytestmark = pytest.mark.gpu

N, NLIST, K, NPROBE = 7_013, 16, 10, 8      # 7,013 = 219 * 32 + 5: the last mask word is partial
BMAX = 256
FORMS = [(64, "f32"), (768, "f32"), (1536, "f32"), (2048, "f16")]
SHARES = {(64, "f32"): True, (768, "f32"): True, (1536, "f32"): True, (2048, "f16"): False}   # 2-byte NITER 4 rows never share lists
LOW = np.uint64(0xFFFFFFFF)


def words_of(mask: np.ndarray, garbage_above: bool = True) -> np.ndarray:
    n = mask.shape[0]
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    words = words.view("<u4").copy()
    if garbage_above and n % 32:
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)   # bits at or above the count are to be ignored
    return words


def key_table(rows_st, dtype, qn):
    """key_of[b, r]: the oracle's packed key of row r for query b (row word = ~r), from exhaustive searches over blocks of 64 rows"""
    n = rows_st.shape[0]
    out = np.zeros((qn.shape[0], n), dtype=np.uint64)
    for a in range(0, n, 64):
        blk = np.ascontiguousarray(rows_st[a : a + 64])
        keys = o.search_keys(blk, dtype, qn, blk.shape[0], a)
        at = (LOW - (keys & LOW)).astype(np.int64)
        np.put_along_axis(out, at, keys, axis=1)
    assert (out != 0).all()
    return out


class Ctx:
    pass


@pytest.fixture(scope="module", params=FORMS, ids=[f"{d}-{t}" for d, t in FORMS])
def ctx(request):
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import native
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    dim, dtype = request.param
    c = Ctx()
    c.torch, c.dim, c.dtype, c.shares = torch, dim, dtype, SHARES[request.param]
    rng = np.random.default_rng(1700 + dim)
    raw = rng.standard_normal((N, dim)).astype(np.float32)
    c.queries = rng.standard_normal((BMAX, dim)).astype(np.float32)
    cent = rng.standard_normal((NLIST, dim)).astype(np.float32)
    # the lists: uneven sizes, list 3 empty, rows in slot order inside a list
    c.assign = rng.choice(np.delete(np.arange(NLIST), 3), size=N, p=np.r_[0.3, 0.2, np.full(NLIST - 3, 0.5 / (NLIST - 3))])
    perm = np.argsort(c.assign, kind="stable").astype(np.int64)
    offsets = np.zeros(NLIST + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(c.assign, minlength=NLIST))
    c.dead = np.zeros(N, dtype=bool)
    c.dead[rng.choice(N, size=N // 8, replace=False)] = True
    c.dead[N - 1] = True

    lib = native.load()
    c.clean, c.deleted = DeviceKnnIndex(dim, dtype), DeviceKnnIndex(dim, dtype)
    for ix in (c.clean, c.deleted):
        ix.upsert(np.arange(N, dtype=np.int64), raw)
        t = [torch.from_numpy(a).to(ix.device) for a in (cent, perm, offsets)]
        native.check(lib.codd_knn_ivf_install(ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), ix._stream()), "codd_knn_ivf_install")
    c.deleted.delete(np.flatnonzero(c.dead))     # after the install: the layout stays valid, its scans mask by the original slot

    qn = o.normalize_rows(c.queries)
    c.key_of = key_table(stored(raw, dtype), dtype, qn)
    _, c.probed = o.search(o.normalize_rows(cent), "f32", qn, NLIST)     # [BMAX, NLIST] lists by exact centroid score, best first
    rng = np.random.default_rng(17)
    block = np.zeros(N, dtype=bool)
    block[2_000:2_777] = True
    few = np.zeros(N, dtype=bool)
    few[[int(perm[offsets[l]]) for l in range(NLIST) if offsets[l + 1] > offsets[l]]] = True   # one row per list: < K in 8 lists
    c.masks = {"half": rng.random(N) < 0.5, "3pct": rng.random(N) < 0.03, "block": block, "few": few}
    yield c
    c.clean.close()
    c.deleted.close()


def reference(c, B, nprobe, mask, dead, row_base=0):
    """[B, K] keys: the K best of key_of among allowed & live & in-the-probed-lists rows, descending, 0 padded"""
    in_lists = np.zeros((B, NLIST), dtype=bool)
    np.put_along_axis(in_lists, c.probed[:B, :nprobe], True, axis=1)
    member = in_lists[:, c.assign] & (mask & ~dead)[None, :]
    keys = np.where(member, c.key_of[:B], np.uint64(0))
    top = np.sort(keys, axis=1)[:, ::-1][:, :K].copy()
    hit = top != 0
    top[hit] -= np.uint64(row_base)              # the row word is ~(row_base + row)
    return top


def masked_keys(c, ix, B, nprobe, mask, row_base=0):
    """keys of the host form and of the device form; asserts they are identical and counted"""
    torch = c.torch
    words = words_of(mask)
    before = ix.stat("ivf_masked_searches")
    host = ix.ivf_search_keys_masked(c.queries[:B], words, K, nprobe, row_base).cpu().numpy().view(np.uint64)
    dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
    dev = ix.ivf_search_keys_masked_dev(c.queries[:B], dev_words, K, nprobe, row_base).cpu().numpy().view(np.uint64)
    assert np.array_equal(host, dev), (B, nprobe, np.flatnonzero((host != dev).any(axis=1))[:8])
    assert ix.stat("ivf_masked_searches") == before + 2
    assert np.array_equal(dev_words.cpu().numpy(), words.view(np.int32)), "the caller's words are left as they were"
    return dev


def variants(c):
    return [(c.clean, np.zeros(N, dtype=bool)), (c.deleted, c.dead)]


@pytest.mark.parametrize("B", [1, BMAX])
def test_exhaustive_probe_equals_the_flat_masked_search_and_the_oracle(ctx, B):
    c = ctx
    for ix, dead in variants(c):
        for name in ("half", "3pct"):
            mask = c.masks[name]
            got = masked_keys(c, ix, B, NLIST, mask, row_base=1_000)
            assert np.array_equal(got, reference(c, B, NLIST, mask, dead, row_base=1_000)), (name, B)
            for route in (1, 2):
                ix.set_option("mask_route", route)
                flat = ix.search_keys_masked(c.queries[:B], words_of(mask), K, 1_000).cpu().numpy().view(np.uint64)
                assert np.array_equal(got, flat), (name, B, route)
            ix.set_option("mask_route", 0)


@pytest.mark.parametrize("B", [1, BMAX])
def test_an_all_ones_mask_gives_the_bits_of_the_unmasked_ivf_search(ctx, B):
    from codd_query_engine_amd import ivf

    c = ctx
    ones = np.ones(N, dtype=bool)
    for ix, dead in variants(c):
        shared0 = ix.stat("ivf_shared_searches")
        plain = ivf.search_ivf_keys(ix, c.queries[:B], K, NPROBE, 77).cpu().numpy().view(np.uint64)
        assert np.array_equal(masked_keys(c, ix, B, NPROBE, ones, row_base=77), plain)
        assert np.array_equal(plain, reference(c, B, NPROBE, ones, dead, row_base=77))
        # the batch takes the scan the unmasked search takes: 2,048 pairs share lists (where the row form shares at all), 8 do not
        assert ix.stat("ivf_shared_searches") - shared0 == (3 if B == BMAX and c.shares else 0)
        d_plain, r_plain = ivf.search_ivf(ix, c.queries[:B], K, NPROBE)
        d_mask, r_mask = ivf.search_ivf(ix, c.queries[:B], K, NPROBE, allow=ones)
        assert c.torch.equal(d_mask, d_plain) and c.torch.equal(r_mask, r_plain)


@pytest.mark.parametrize("B", [1, BMAX])
@pytest.mark.parametrize("name", ["half", "3pct", "block", "few"])
def test_partial_probe_answers_from_the_allowed_live_rows_of_the_probed_lists(ctx, name, B):
    c = ctx
    mask = c.masks[name]
    for ix, dead in variants(c):
        ref = reference(c, B, NPROBE, mask, dead)
        got = masked_keys(c, ix, B, NPROBE, mask)
        assert np.array_equal(got, ref), (name, B, np.flatnonzero((got != ref).any(axis=1))[:8])
        if name == "few":
            assert (ref[:, K - 1] == 0).all() and (ref[:, 0] != 0).any()       # fewer than K allowed rows in 8 lists: padding
    # ... and the distances / rows outputs are the keys unpacked (device form, through ivf.search_ivf)
    from codd_query_engine_amd import ivf

    dev_words = c.torch.from_numpy(words_of(mask).view(np.int32)).to(c.deleted.device)
    dist, rows = ivf.search_ivf(c.deleted, c.queries[:B], K, NPROBE, allow=dev_words)
    d_ref, r_ref = o.unpack_keys(reference(c, B, NPROBE, mask, c.dead))
    assert np.array_equal(rows.cpu().numpy(), r_ref) and np.array_equal(dist.cpu().numpy(), d_ref)
    dist, rows = ivf.search_ivf(c.deleted, c.queries[:B], K, NPROBE, allow=mask)       # host form, from a bool array
    assert np.array_equal(rows.cpu().numpy(), r_ref) and np.array_equal(dist.cpu().numpy(), d_ref)


def test_the_batch_scan_shares_lists_under_a_mask(ctx):
    c = ctx
    before = c.clean.stat("ivf_shared_searches")
    masked_keys(c, c.clean, BMAX, NPROBE, c.masks["half"])       # 2,048 pairs >= 1,024 and >= 2 * 16 lists
    assert c.clean.stat("ivf_shared_searches") - before == (2 if c.shares else 0)
    masked_keys(c, c.clean, 1, NPROBE, c.masks["half"])          # 8 pairs: the per-pair scan, lists split over workgroups
    assert c.clean.stat("ivf_shared_searches") - before == (2 if c.shares else 0)


@pytest.mark.parametrize("B", [1, BMAX])
def test_an_empty_mask_gives_an_all_empty_result(ctx, B):
    c = ctx
    for ix, _ in variants(c):
        assert (masked_keys(c, ix, B, NPROBE, np.zeros(N, dtype=bool)) == 0).all()
    dist, rows = c.clean.ivf_search_masked_dev_tensors(c.queries[:B], c.torch.zeros(((N + 31) // 32,), dtype=c.torch.int32, device=c.clean.device), K, NPROBE)
    assert bool((rows == -1).all()) and bool(c.torch.isinf(dist).all())
    only_dead = c.dead.copy()                                     # every allowed row is deleted: empty as well
    assert (masked_keys(c, c.deleted, B, NLIST, only_dead) == 0).all()


def test_the_device_words_are_read_on_the_stream_behind_what_wrote_them(ctx):
    """Ordering only: the mask is produced by torch ops enqueued on the same stream just before the call and nobody synchronises;
    the entry point reads nothing back, so the words do not exist yet when it returns."""
    c = ctx
    torch = c.torch
    a = np.random.default_rng(7).random(N) < 0.5
    b = np.random.default_rng(8).random(N) < 0.5
    wa = torch.from_numpy(words_of(a).view(np.int32)).to(c.deleted.device)
    wb = torch.from_numpy(words_of(b, garbage_above=False).view(np.int32)).to(c.deleted.device)
    side = torch.cuda.Stream(device=c.deleted.device)
    side.wait_stream(torch.cuda.current_stream(c.deleted.device))
    with torch.cuda.stream(side):
        for B in (1, BMAX):
            words = wa & ~wb
            keys = c.deleted.ivf_search_keys_masked_dev(c.queries[:B], words, K, NPROBE)
            words.zero_()                                          # behind the search on the stream: it must not see this
            side.synchronize()
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), reference(c, B, NPROBE, a & ~b, c.dead)), B


def test_bad_arguments_are_einval(ctx):
    from codd_query_engine_amd import native
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    c = ctx
    torch = c.torch
    nwords = (N + 31) // 32
    for wrong in (nwords - 1, nwords + 1):
        with pytest.raises(native.NativeLibraryError, match="-22"):
            c.clean.ivf_search_keys_masked(c.queries[:1], np.zeros(wrong, dtype=np.uint32), K, NPROBE)
        with pytest.raises(native.NativeLibraryError, match="-22"):
            c.clean.ivf_search_keys_masked_dev(c.queries[:1], torch.zeros((wrong,), dtype=torch.int32, device=c.clean.device), K, NPROBE)
    with pytest.raises(ValueError):
        c.clean.ivf_search_keys_masked_dev(c.queries[:1], np.zeros(nwords, dtype=np.uint32), K, NPROBE)   # host words belong to the host form
    # no layout, and a layout gone stale through an upsert
    rng = np.random.default_rng(5)
    n, nlist = 203, 4
    raw = rng.standard_normal((n, c.dim)).astype(np.float32)
    ix = DeviceKnnIndex(c.dim, c.dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ones = np.ones(n, dtype=bool)
    dev_ones = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=ix.device)
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.ivf_search_keys_masked(raw[:1], ones, K, 2)
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.ivf_search_keys_masked_dev(raw[:1], dev_ones, K, 2)
    assign = np.arange(n) % nlist
    perm = np.argsort(assign, kind="stable").astype(np.int64)
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    t = [torch.from_numpy(a).to(ix.device) for a in (raw[:nlist].copy(), perm, offsets)]
    native.check(native.load().codd_knn_ivf_install(ix._h, t[0].data_ptr(), nlist, t[1].data_ptr(), t[2].data_ptr(), ix._stream()), "codd_knn_ivf_install")
    flat = ix.search_keys_masked(raw[:3], ones, K).cpu().numpy()
    assert np.array_equal(ix.ivf_search_keys_masked(raw[:3], ones, K, nlist).cpu().numpy(), flat)
    assert np.array_equal(ix.ivf_search_keys_masked_dev(raw[:3], dev_ones, K, nlist).cpu().numpy(), flat)
    ix.upsert(np.array([7], dtype=np.int64), raw[:1])
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.ivf_search_keys_masked(raw[:1], ones, K, 2)
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.ivf_search_keys_masked_dev(raw[:1], dev_ones, K, 2)
    ix.close()
