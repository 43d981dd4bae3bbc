"""Every device buffer, pinned buffer and event of an index has one owner that frees it (csrc/device_mem.h).

The library counts what it holds (codd_knn_debug_live_allocations: buffers, bytes, events, process-wide).  Each test reads the
counters first and compares against that baseline, never against zero: indexes of other tests may be alive.  Small shapes on
purpose (dim 64, a few thousand rows): who frees what does not depend on size; options force the routes at this size and the
stats say which route ran."""

import ctypes
import gc

import numpy as np
import pytest

from codd_query_engine_amd import ivf, native

pytestmark = pytest.mark.gpu

D, K = 64, 5


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex


def live():
    gc.collect()  # (an index some earlier test dropped without close() goes now, not in the middle of this test)
    return native.live_allocations()


def new_index(Index):
    ix = Index(D, "f16")
    ix.set_option("filter_min_rows", 1)
    ix.set_option("filter_min_rows_small", 1)   # a single query takes the filter at this size too
    ix.set_option("shadow8_max_batch", 64)      # up to 64 queries: the int8 filter; above: the 2-byte filter
    ix.set_option("hit_cap", 8192)              # (more than the rows there are: nothing is truncated, and the workspaces stay small)
    return ix


def rand(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, D), generator=g, device="cuda")


def exact(ix, q):
    ix.set_option("filter", 0)
    out = ix.search_tensors(q, K)
    ix.set_option("filter", 1)
    return out


def same(torch, a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def install(torch, ix, nlist, perm=None, offsets=None):
    """codd_knn_ivf_install of an arbitrary partition (row r in list r % nlist): with nprobe = nlist the IVF search is the flat
    search.  Returns the call's code."""
    n = ix.count()
    cent = rand(torch, nlist, 99)
    if perm is None:
        perm = torch.sort(torch.arange(n, device="cuda") % nlist, stable=True).indices.contiguous()
    if offsets is None:
        sizes = torch.bincount(torch.arange(n, device="cuda") % nlist, minlength=nlist)
        offsets = torch.zeros(nlist + 1, dtype=torch.int64, device="cuda")
        offsets[1:] = torch.cumsum(sizes, 0)
    rc = native.load().codd_knn_ivf_install(ix._h, cent.data_ptr(), nlist, perm.data_ptr(), offsets.data_ptr(), ix._stream())
    torch.cuda.synchronize()
    return rc, perm, offsets


def test_everything_is_given_back(env):
    torch, Index = env
    base = live()
    n = 6000
    x = rand(torch, n, 1)
    ix = new_index(Index)
    ix.upsert(np.arange(1000, dtype=np.int64), x[:1000].cpu().numpy())
    ix.upsert_device(1000, x[1000:].contiguous())
    q1, q300 = rand(torch, 1, 2), rand(torch, 300, 3)
    r1, r300 = ix.search_tensors(q1, K), ix.search_tensors(q300, K)
    assert ix.stat("shadow8_builds") == 1 and ix.stat("shadow16_builds") == 1
    assert same(torch, r1, exact(ix, q1)) and same(torch, r300, exact(ix, q300))

    ix.set_scopes(np.arange(n, dtype=np.int64), (np.arange(n) % 3 + 1).astype(np.uint32))
    _, rows = ix.search_scoped_tensors(rand(torch, 4, 4), np.array([1, 2, 3, 0], dtype=np.uint32), K)
    assert ix.stat("scoped_searches") == 1 and ix.stat("scope_builds") == 1
    assert all(int(r) % 3 + 1 == s for s, row in zip((1, 2, 3), rows.tolist()) for r in row)

    ix.delete(np.arange(0, n, 7, dtype=np.int64))
    assert ix.stat("dead_rows") == (n + 6) // 7

    allow = np.zeros(n, dtype=bool)
    allow[::2] = True
    words = ix._allow_words(allow)
    dev_words = torch.from_numpy(words.view(np.int32).copy()).cuda()
    q8 = rand(torch, 8, 5)
    answers = []
    for route in (1, 2):
        ix.set_option("mask_route", route)
        answers.append(ix.search_masked_tensors(q8, allow, K))
        answers.append(ix.search_masked_dev_tensors(q8, dev_words, K))
    ix.set_option("mask_route", 0)
    assert ix.stat("mask_list_searches") == 2 and ix.stat("mask_dense_searches") == 2 and ix.stat("masked_dev_searches") == 2
    assert all(same(torch, a, answers[0]) for a in answers[1:])
    assert all(r % 2 == 0 and r % 7 != 0 for row in answers[0][1].tolist() for r in row)

    ix.set_documents([b"row %d" % r for r in range(n)])
    bits = ix.match_documents(b"row 41")
    assert ix.stat("doc_matches") == 1
    hit = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:n].nonzero()[0].tolist()
    assert hit == [r for r in range(n) if str(r).startswith("41")]

    nlist = 8
    rc, _, _ = install(torch, ix, nlist)
    assert rc == 0
    flat1, flat300 = ix.search_tensors(q1, K), ix.search_tensors(q300, K)
    assert same(torch, ivf.search_ivf(ix, q1, K, nlist), flat1)                     # per (query, list) pair
    shared = ix.stat("ivf_shared_searches")
    assert same(torch, ivf.search_ivf(ix, q300, K, nlist), flat300)                 # 2,400 pairs: every list scanned once
    assert ix.stat("ivf_shared_searches") == shared + 1
    assert same(torch, ivf.search_ivf(ix, q8, K, nlist, allow=allow), answers[0])   # under the mask
    assert ix.stat("ivf_masked_searches") == 1

    assert ix.compact() == n - (n + 6) // 7 and ix.stat("compactions") == 1

    now = live()
    assert now[0] > base[0] and now[1] > base[1] and now[2] > base[2]
    ix.close()
    assert live() == base


def test_regrowth_frees_what_it_replaces(env):
    torch, Index = env
    base = live()
    n0 = 5000
    ix = new_index(Index)
    ix.upsert_device(0, rand(torch, n0, 11))
    q1, q300 = rand(torch, 1, 12), rand(torch, 300, 13)

    def append_and_search(seed):
        # a fifth more rows: past the shadows' head room of an eighth, so both are allocated again
        m = ix.count() // 5
        builds = ix.stat("shadow8_builds"), ix.stat("shadow16_builds")
        bytes_before = ix.stat("device_bytes")
        ix.upsert_device(ix.count(), rand(torch, m, seed))
        r1, r300 = ix.search_tensors(q1, K), ix.search_tensors(q300, K)
        assert (ix.stat("shadow8_builds"), ix.stat("shadow16_builds")) == (builds[0] + 1, builds[1] + 1)
        assert ix.stat("device_bytes") > bytes_before
        assert same(torch, r1, exact(ix, q1)) and same(torch, r300, exact(ix, q300))
        return live()

    ix.search_tensors(q1, K), ix.search_tensors(q300, K), exact(ix, q300)
    first = append_and_search(14)
    second = append_and_search(15)
    assert second[0] == first[0] and second[2] == first[2] and second[1] > first[1]

    n = ix.count()
    ix.set_documents([b"a" * (r % 5) for r in range(n)])
    first = live()
    ix.set_documents([b"b" * (r % 50) for r in range(n)])
    second = live()
    assert second[0] == first[0] and second[2] == first[2] and second[1] > first[1]

    counts = []
    for nlist in (4, 8):
        rc, _, _ = install(torch, ix, nlist)
        assert rc == 0
        assert same(torch, ivf.search_ivf(ix, q300, K, nlist), exact(ix, q300))
        counts.append(live())
    assert counts[1][0] == counts[0][0] and counts[1][2] == counts[0][2]

    allow = np.ones(n, dtype=bool)
    allow[::3] = False
    ix.set_option("mask_route", 1)
    counts = []
    side = torch.cuda.Stream()   # (a stream of its own: a fresh workspace, so the larger batch has buffers to outgrow)
    torch.cuda.synchronize()
    for B in (8, 64):
        q = rand(torch, B, 16)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _, rows = ix.search_masked_tensors(q, allow, K)
        side.synchronize()
        assert ix.stat("last_mask_rows") == int(allow.sum()) and all(r % 3 != 0 for row in rows.tolist() for r in row)
        counts.append(live())
    assert ix.stat("mask_list_searches") == 2
    assert counts[1][0] == counts[0][0] and counts[1][2] == counts[0][2] and counts[1][1] > counts[0][1]

    ix.close()
    assert live() == base


def test_failed_calls_leave_nothing_behind(env):
    torch, Index = env
    base = live()
    n = 4000
    ix = new_index(Index)
    ix.upsert_device(0, rand(torch, n, 21))
    q1, q300 = rand(torch, 1, 22), rand(torch, 300, 23)
    # everything the answers below need exists before the calls that fail: the filter workspace and the int8 shadow (one
    # query), the exact scan's buffers for 300 queries
    ix.search_tensors(q1, K)
    want300 = exact(ix, q300)
    assert ix.stat("shadow8_builds") == 1 and ix.stat("shadow16_builds") == 0

    nlist = 8
    before = live()
    bad_offsets = torch.arange(nlist + 1, dtype=torch.int64, device="cuda") * (n // nlist - 1)   # ends below the count
    rc, perm, offsets = install(torch, ix, nlist, offsets=bad_offsets)
    assert rc == -22 and "offsets" in native.last_error() and live() == before
    bad_perm = torch.sort(torch.arange(n, device="cuda") % nlist, stable=True).indices.contiguous()
    bad_perm[n // 2] = n   # one entry out of range
    rc, _, _ = install(torch, ix, nlist, perm=bad_perm)
    assert rc == -22 and "permutation" in native.last_error() and live() == before
    with pytest.raises(native.NativeLibraryError):
        ivf.search_ivf(ix, q1, K, nlist)   # no layout was left behind
    assert same(torch, ix.search_tensors(q300[:40].contiguous(), K), (want300[0][:40], want300[1][:40]))

    before = live()
    ix.set_option("debug_fail_shadow_alloc", 1)
    got = ix.search_tensors(q300, K)   # 300 queries want the 2-byte shadow; without it, and above the int8 batch limit: the exact scan
    assert ix.stat("shadow16_alloc_failures") == 1 and ix.stat("shadow16_builds") == 0
    assert same(torch, got, want300) and live() == before
    ix.set_option("debug_fail_shadow_alloc", 0)
    assert same(torch, ix.search_tensors(q300, K), want300) and ix.stat("shadow16_builds") == 1

    ix.close()
    assert live() == base


def test_workspaces_change_hands_without_sharing(env):
    torch, Index = env
    base = live()
    ix = new_index(Index)
    ix.upsert_device(0, rand(torch, 4000, 31))
    q = rand(torch, 16, 32)
    want = ix.search_tensors(q, K)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(5)]   # one more than an index keeps workspaces: the least recently used changes hands
    for _ in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                got = ix.search_tensors(q, K)
            s.synchronize()
            assert same(torch, got, want)
    assert ix.stat("workspaces") == 4
    ix.close()
    assert live() == base
