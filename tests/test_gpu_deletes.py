"""Tombstones and compaction on the GPU, through the C ABI (codd_knn_delete_host / _live_count / _compact).
The expected answer of every query is the oracle's search over the LIVE rows only (row order kept, so "ties -> lower row"
carries over), its indices mapped back to row slots through the monotone map np.flatnonzero(live).  Every comparison is bit for
bit on row ids and fp32 distances, padding included: no tolerance, no query left out.  Each search path is forced through the
existing options and confirmed through the existing stats."""

import os
import subprocess
import sys

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests._deleting_oracle_engine import live_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deletes_untouched_parent")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex, ivf


def stored(raw, dtype):
    return o.to_storage(o.normalize_rows(raw), dtype)


def always_filter(ix):
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)
    ix.set_option("shadow8_cooldown", 0)   # (a crowded pass must not move the next search to another filter: the tests name the path)


def check(ix, rows_ref, dtype, live, q, k, what=""):
    d_ref, r_ref = live_reference(rows_ref, dtype, np.flatnonzero(live), o.normalize_rows(q), k)
    dist, rows = ix.search(q, k)
    bad = np.flatnonzero((rows != r_ref).any(axis=1))
    assert bad.size == 0, (what, dtype, q.shape, k, bad[:8], rows[bad[:1]], r_ref[bad[:1]])
    assert np.array_equal(dist, d_ref), (what, dtype, q.shape, k)
    return dist, rows


def expected_keys(rows_ref, dtype, live, q, k, row_base):
    """packed keys of the live sub-matrix with the slots mapped back (and row_base added)"""
    members = np.flatnonzero(live)
    keys = np.zeros((q.shape[0], k), dtype=np.uint64)
    if members.size == 0:
        return keys
    sub = o.search_keys(np.ascontiguousarray(rows_ref[members]), dtype, o.normalize_rows(q), k, 0)
    hit = sub != 0
    local = (np.uint64(0xFFFFFFFF) - (sub[hit] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    rows = (members[local] + row_base).astype(np.uint64)
    keys[hit] = (sub[hit] & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - rows)
    return keys


def planted(rng, n, dim, B, dups=10):
    """raw rows, queries, and per query `dups` planted near-duplicates (best first) at random slots >= 2000"""
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    slots = 2000 + rng.permutation(n - 2000)[: B * dups].reshape(B, dups)   # (behind the leading tiles the tests delete wholesale)
    for b in range(B):
        for j in range(dups):
            raw[slots[b, j]] = q[b] + (0.02 + 0.02 * j) * rng.standard_normal(dim).astype(np.float32)
    return raw, q, slots


# ------------------------------------------------------------------------------------------------------------------------
# every search path, with the adversarial deletes in place: per query the best 5 of 10 planted near-duplicates are dead (the
# threshold anchors and finalize's first k would all be dead rows), four whole leading tiles are dead (tile 0 is always sampled),
# 1 % of the rows at random, and one deleted row ties exactly with a live one
# ------------------------------------------------------------------------------------------------------------------------
PATHS = [
    # name, dtype, dim, n, B, filter forced on whatever the size, options, stat that must move
    ("scan_small", "f32", 768, 12_000, 8, False, {}, "scan_launches"),
    ("scan_off", "bf16", 384, 30_000, 40, False, {"filter": 0}, "scan_launches"),
    ("scan_k128", "f16", 384, 9_000, 5, False, {"filter": 0}, "scan_launches"),
    ("bf16_gemm", "f32", 768, 60_000, 40, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes"),
    ("bf16_gemm_b200", "bf16", 384, 40_000, 200, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes"),
    ("f16_tile", "f32", 768, 40_000, 200, True, {"shadow8": 0}, "f16_tile_passes"),
    ("i8_gen1", "f32", 768, 60_000, 40, True, {"i8v2": 0}, "shadow8_passes"),
    ("i8_gen1_f16", "f16", 384, 60_000, 20, True, {"i8v2": 0}, "shadow8_passes"),
    ("i8_tile_half", "f32", 768, 40_000, 100, True, {}, "i8v2_passes"),
    ("i8_tile", "f32", 768, 40_000, 256, True, {}, "i8v2_passes"),
    ("i8_tile_bf16", "bf16", 768, 40_000, 140, True, {}, "i8v2_passes"),
    ("fallback", "f32", 768, 40_000, 140, True, {"hit_cap": 16}, "fallback_queries"),
    ("fallback_unfused", "f32", 768, 60_000, 40, True, {"hit_cap": 16}, "fallback_queries"),
    ("small_batch", "f32", 768, 40_000, 1, True, {"small_batch_max": 1}, "small_batch_passes"),
    ("wide_f32_1536", "f32", 1536, 12_000, 8, False, {}, "scan_launches"),
    ("wide_f32_1536_filter", "f32", 1536, 40_000, 140, True, {}, "filter_passes"),
    ("wide_bf16_4096", "bf16", 4096, 6_000, 6, False, {}, "scan_launches"),
    ("wide_bf16_4096_filter", "bf16", 4096, 20_000, 40, True, {}, "filter_passes"),
]


@pytest.mark.parametrize("name,dtype,dim,n,B,forced,options,moved", PATHS, ids=[p[0] for p in PATHS])
def test_every_path_returns_the_exact_top_k_of_the_live_rows(env, name, dtype, dim, n, B, forced, options, moved):
    _, Index, _ = env
    rng = np.random.default_rng(len(name) * 1000 + dim + B)
    raw, q, slots = planted(rng, n, dim, B)
    free = np.setdiff1d(np.arange(2000, n), slots.ravel())
    a, b = int(free[10]), int(free[400])
    raw[b] = raw[a]                                   # an exact tie: the earlier row will be deleted
    q[-1] = raw[a]
    ix = Index(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    if forced:
        always_filter(ix)
    for key, value in options.items():
        ix.set_option(key, value)
    rows_ref = stored(raw, dtype)
    live = np.ones(n, dtype=bool)
    ks = (128,) if name == "scan_k128" else (10, 100) if B <= 40 and dim <= 768 else (10,)
    check(ix, rows_ref, dtype, live, q, 10, name + " before")    # (also builds the shadows: a delete must not need them rebuilt)
    builds = (ix.stat("shadow8_builds"), ix.stat("shadow16_builds"))
    others = np.setdiff1d(free, [a, b])
    dead = np.concatenate([slots[:, :5].ravel(), np.arange(1024), rng.permutation(others)[: n // 100], [a]])
    ix.delete(dead)
    live[dead] = False
    assert ix.count() == n and ix.live_count() == int(live.sum()) == n - ix.stat("dead_rows") and ix.stat("delete_calls") == 1
    before, passes = ix.stat(moved), ix.stat("filter_passes") + ix.stat("small_batch_passes")
    for k in ks:
        dist, rows = check(ix, rows_ref, dtype, live, q, k, name)
        assert not np.isin(rows, dead).any()
        assert rows[-1, 0] == b and dist[-1, 0] == live_reference(rows_ref, dtype, np.array([a]), o.normalize_rows(q[-1:]), 1)[0][0, 0]
        if B > 1:
            # (which of two neighbouring planted rows scores higher is up to their noise: compared as sets, the oracle fixed the order above)
            assert (np.sort(rows[:-1, :5], axis=1) == np.sort(slots[:-1, 5:], axis=1)).all(), "the five surviving planted rows lead"
    assert ix.stat(moved) > before, (name, moved)
    if forced and n >= 60_000:   # (enough sample tiles for k = 100 as well: two list slots per lane in the anchors and in finalize)
        assert ix.stat("filter_passes") + ix.stat("small_batch_passes") == passes + len(ks), name
    assert (ix.stat("shadow8_builds"), ix.stat("shadow16_builds")) == builds, "a delete leaves both shadows as they are"
    ix.close()


def test_padding_when_fewer_than_k_rows_live_and_empty_answers_when_none_does(env):
    _, Index, _ = env
    rng = np.random.default_rng(21)
    n, dim, k = 40_000, 768, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rows_ref = stored(raw, "f32")
    for B, options, moved in ((4, {"filter": 0}, "scan_launches"), (140, {}, "i8v2_passes"), (40, {"shadow8": 0}, "filter_passes"),
                              (140, {"hit_cap": 16}, "fallback_queries"), (1, {"small_batch_max": 1}, "small_batch_passes")):
        ix = Index(dim, dtype="f32")
        ix.upsert(np.arange(n, dtype=np.int64), raw)
        always_filter(ix)
        for key, value in options.items():
            ix.set_option(key, value)
        q = rng.standard_normal((B, dim)).astype(np.float32)
        keep = rng.permutation(n)[: k - 1]
        live = np.zeros(n, dtype=bool)
        live[keep] = True
        ix.delete(np.flatnonzero(~live))
        assert ix.live_count() == k - 1 and ix.count() == n
        before = ix.stat(moved)
        dist, rows = check(ix, rows_ref, "f32", live, q, k, f"k-1 live {options}")
        assert (rows[:, : k - 1] >= 0).all() and (rows[:, k - 1] == -1).all() and np.isinf(dist[:, k - 1]).all()
        assert ix.stat(moved) > before
        ix.delete(keep)
        ix.delete(keep[:3])                                          # dead already: a no-op
        assert ix.live_count() == 0 and ix.stat("dead_rows") == n and ix.stat("delete_calls") == 3
        dist, rows = check(ix, rows_ref, "f32", np.zeros(n, dtype=bool), q, k, f"all dead {options}")
        assert (rows == -1).all() and np.isinf(dist).all()
        ix.close()


def test_search_keys_with_a_row_base(env):
    torch, Index, _ = env
    rng = np.random.default_rng(22)
    n, dim, B, base = 40_000, 768, 140, 3_000_000
    raw, q, slots = planted(rng, n, dim, B)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    live = np.ones(n, dtype=bool)
    live[slots[:, :5].ravel()] = False
    live[rng.permutation(n)[:500]] = False
    ix.delete(np.flatnonzero(~live))
    for queries, filt in ((q, 1), (q[:3], 0)):                       # the int8 tile filter, then the exact scan
        ix.set_option("filter", filt)
        for k in (10, 30) if filt else (10, 100):                    # (k = 100 needs more sample tiles than 40,000 rows have)
            keys = ix.search_keys(queries, k, row_base=base).cpu().numpy().view(np.uint64)
            assert np.array_equal(keys, expected_keys(rows_ref, "f32", live, queries, k, base)), (queries.shape, k)
    assert ix.stat("i8v2_passes") == 2 and ix.stat("scan_launches") >= 2
    ix.close()


def test_scoped_search_mixed_with_scope_zero(env):
    _, Index, _ = env
    rng = np.random.default_rng(23)
    n, dim = 20_000, 384
    for dtype in ("f32", "bf16", "f16"):
        raw = rng.standard_normal((n, dim)).astype(np.float32)
        labels = rng.integers(0, 5, n).astype(np.uint32)
        labels[5000:7000] = 4                                        # one contiguous namespace: whole waves of one scope
        ix = Index(dim, dtype=dtype)
        ix.upsert(np.arange(n, dtype=np.int64), raw)
        ix.set_scopes(np.arange(n, dtype=np.int64), labels)
        rows_ref = stored(raw, dtype)
        q = rng.standard_normal((64, dim)).astype(np.float32)
        scopes = (np.arange(64) % 6).astype(np.uint32)               # 0 .. 5; nobody carries 5
        live = np.ones(n, dtype=bool)

        def check_scoped(k):
            dist, rows = ix.search_scoped(q, scopes, k)
            for s in range(6):
                member = live if s == 0 else live & (labels == s)
                sel = np.flatnonzero(scopes == s)
                d_ref, r_ref = live_reference(rows_ref, dtype, np.flatnonzero(member), o.normalize_rows(q[sel]), k)
                assert np.array_equal(rows[sel], r_ref) and np.array_equal(dist[sel], d_ref), (dtype, s, k)

        check_scoped(10)
        builds = ix.stat("scope_builds")
        dead = np.concatenate([rng.permutation(n)[:3000], np.arange(5100, 5900), np.flatnonzero(labels == 3)[7:]])   # scope 3 keeps 7 rows (< k)
        ix.delete(dead)
        live[dead] = False
        for k in (10, 100):
            check_scoped(k)
        assert ix.stat("scope_builds") == builds + 1, "a delete marks the lists for one rebuild"
        with pytest.raises(native.NativeLibraryError):
            ix.set_scopes(dead[:1].astype(np.int64), np.array([2], dtype=np.uint32))
        ix.close()


@pytest.mark.parametrize("dtype,dim,B", [("f32", 128, 9), ("f16", 128, 64), ("bf16", 1536, 9), ("f32", 1536, 64)])
def test_ivf_layout_installed_before_the_deletes_stays_valid(env, dtype, dim, B):
    torch, Index, ivf = env
    rng = np.random.default_rng(24 + dim + B)
    n, nlist = 20_000, 32
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ivf.build_ivf(ix, nlist, iters=3)
    rows_ref = stored(raw, dtype)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    q[0] = raw[77]
    live = np.ones(n, dtype=bool)
    dead = np.concatenate([rng.permutation(n)[:2000], [77]])
    ix.delete(dead)
    live[dead] = False
    shared = ix.stat("ivf_shared_searches")
    for k in (10, 100):
        d_ref, r_ref = live_reference(rows_ref, dtype, np.flatnonzero(live), o.normalize_rows(q), k)
        d, r = ivf.search_ivf(ix, torch.from_numpy(q).cuda(), k, nprobe=nlist)
        assert np.array_equal(r.cpu().numpy(), r_ref) and np.array_equal(d.cpu().numpy(), d_ref), (dtype, dim, B, k)
    assert (ix.stat("ivf_shared_searches") > shared) == (B * nlist >= 1024)
    ix.close()


def test_delete_then_upsert_then_delete_again_and_two_streams(env):
    torch, Index, _ = env
    rng = np.random.default_rng(25)
    n, dim, B = 40_000, 768, 140
    raw = rng.standard_normal((n + 3000, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    raw[[5, 9000, 39_999, n + 10, n + 2999]] = q[:5] + 0.01        # planted best matches, old and new rows
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw[:n])
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    live = np.zeros(n + 3000, dtype=bool)
    live[:n] = True
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        d1, r1 = ix.search_tensors(qd, 10)                          # in flight on stream 1 ...
    ix.delete(np.array([5, 9000, 123, 124], dtype=np.int64))        # ... the delete waits for it (exclusive, synchronous)
    live[[5, 9000, 123, 124]] = False
    with torch.cuda.stream(s2):
        d2, r2 = ix.search_tensors(qd, 10)
    torch.cuda.synchronize()
    d_ref, r_ref = live_reference(rows_ref, "f32", np.arange(n), o.normalize_rows(q), 10)
    assert np.array_equal(r1.cpu().numpy(), r_ref) and np.array_equal(d1.cpu().numpy(), d_ref)
    d_ref, r_ref = live_reference(rows_ref, "f32", np.flatnonzero(live), o.normalize_rows(q), 10)
    assert np.array_equal(r2.cpu().numpy(), r_ref) and np.array_equal(d2.cpu().numpy(), d_ref)
    assert ix.stat("workspaces") >= 2
    # new rows behind the old ones (the row store and the bitmap grow), then deletes among old and new
    ix.upsert(np.arange(n, n + 3000, dtype=np.int64), raw[n:])
    live[n:] = True
    check(ix, rows_ref, "f32", live, q, 10, "after upsert")
    again = np.concatenate([[39_999, n + 10, 5], rng.permutation(n + 3000)[:400]])
    ix.delete(again)
    live[again] = False
    assert ix.live_count() == int(live.sum()) and ix.count() == n + 3000
    check(ix, rows_ref, "f32", live, q, 10, "after second delete")
    check(ix, rows_ref, "f32", live, q[:4], 100, "after second delete, scan")
    ix.close()


def test_error_contracts(env):
    _, Index, _ = env
    rng = np.random.default_rng(26)
    n, dim = 5000, 384
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    want = ix.search(q, 10)
    for bad in ([10, n], [-1], [3, 10**12]):
        with pytest.raises(native.NativeLibraryError, match="-22"):
            ix.delete(np.array(bad, dtype=np.int64))
    assert ix.live_count() == n and ix.stat("dead_rows") == 0 and ix.stat("delete_calls") == 0
    got = ix.search(q, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ix.delete(np.array([], dtype=np.int64))
    ix.delete(np.array([7, 7, 4000], dtype=np.int64))                # a repeated slot counts once
    assert ix.live_count() == n - 2
    before = ix.read_rows(0, n)
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.upsert(np.array([6, 7], dtype=np.int64), raw[:2])
    import torch

    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.upsert_device(3990, torch.from_numpy(raw[:20]).cuda())
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.load_rows(before[:5], first_slot=3998)
    assert np.array_equal(ix.read_rows(0, n), before), "a refused write changes nothing"
    assert np.array_equal(before[7], stored(raw[7:8], "f32")[0]), "read_rows is slot-addressed: a dead slot's contents stay readable"
    ix.upsert(np.array([6, 8, n], dtype=np.int64), raw[:3])          # live slots and a new one are writable as ever
    assert ix.count() == n + 1 and ix.live_count() == n - 1
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# compaction
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim,n,chunk,front", [("f32", 768, 40_000, 0, False), ("f32", 768, 40_000, 1000, True), ("bf16", 384, 30_000, 37, False),
                                                     ("f16", 384, 30_000, 4096, True), ("bf16", 4096, 6_000, 100, True), ("f32", 1536, 12_000, 0, False)])
def test_compact_is_the_stable_squeeze_and_every_path_answers_as_before(env, dtype, dim, n, chunk, front):
    torch, Index, ivf = env
    rng = np.random.default_rng(27 + dim + n + chunk)
    B = 140
    raw, q, slots = planted(rng, n, dim, B, dups=4)
    labels = rng.integers(0, 4, n).astype(np.uint32)
    ix = Index(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ix.set_scopes(np.arange(n, dtype=np.int64), labels)
    always_filter(ix)
    ix.set_option("compact_chunk_rows", chunk)                      # (0: what 64 MiB hold; else more live rows than one bounce buffer)
    ivf.build_ivf(ix, 16, iters=2)
    old = ix.read_rows(0, n)
    assert np.array_equal(old, stored(raw, dtype))
    ix.search(q, 10)                                                # both the int8 shadow and the scope lists exist before the squeeze
    if front:   # dead rows clustered at the front: every later row moves far down, sources and destinations of a chunk overlap
        dead = np.concatenate([np.arange(0, n // 3), n // 3 + rng.permutation(n - n // 3)[:200], slots[:, 0]])
    else:
        dead = np.concatenate([rng.permutation(n)[: n // 10], slots[:, 0], np.arange(n - 300, n)])
    ix.delete(dead)
    live = np.ones(n, dtype=bool)
    live[dead] = False
    keep = np.flatnonzero(live)
    want = check(ix, old, dtype, live, q, 10, "tombstoned")
    d_ivf, r_ivf = ivf.search_ivf(ix, torch.from_numpy(q[:9]).cuda(), 10, nprobe=16)
    assert ix.compact() == keep.size
    assert ix.count() == ix.live_count() == keep.size and ix.stat("dead_rows") == 0 and ix.stat("compactions") == 1
    new = ix.read_rows(0, keep.size)
    assert np.array_equal(new, old[keep]), "live rows in slot order, bit for bit"
    with pytest.raises(native.NativeLibraryError):
        ix.read_rows(0, keep.size + 1)
    all_live = np.ones(keep.size, dtype=bool)
    # the same answers, renumbered by the monotone map — on the int8 tile filter, the first-generation kernels, the 2-byte filter, the scan
    got = check(ix, new, dtype, all_live, q, 10, "compacted i8 tile")
    assert np.array_equal(keep[got[1]], want[1]) and np.array_equal(got[0], want[0])
    check(ix, new, dtype, all_live, q[:40], 100, "compacted i8 gen1")
    check(ix, new, dtype, all_live, q[:1], 10, "compacted single query")
    ix.set_option("shadow8", 0)
    check(ix, new, dtype, all_live, q, 10, "compacted 2-byte filter")
    ix.set_option("filter", 0)
    check(ix, new, dtype, all_live, q[:8], 10, "compacted scan")
    ix.set_option("filter", 1)
    ix.set_option("shadow8", 1)
    # scopes followed the rows
    scopes = (np.arange(B) % 4).astype(np.uint32)
    dist, rows = ix.search_scoped(q, scopes, 10)
    for s in range(4):
        member = np.flatnonzero(labels[keep] == s) if s else np.arange(keep.size)
        sel = np.flatnonzero(scopes == s)
        d_ref, r_ref = live_reference(new, dtype, member, o.normalize_rows(q[sel]), 10)
        assert np.array_equal(rows[sel], r_ref) and np.array_equal(dist[sel], d_ref), s
    # the IVF layout is stale until it is installed again; then it answers like the flat search
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ivf.search_ivf(ix, torch.from_numpy(q[:9]).cuda(), 10, nprobe=16)
    ivf.build_ivf(ix, 16, iters=2)
    d2, r2 = ivf.search_ivf(ix, torch.from_numpy(q[:9]).cuda(), 10, nprobe=16)
    assert np.array_equal(keep[r2.cpu().numpy()], r_ivf.cpu().numpy()) and torch.equal(d2, d_ivf)
    # twice is a no-op; the freed slots are new slots again (no label, writable)
    assert ix.compact() == keep.size and ix.stat("compactions") == 1
    extra = rng.standard_normal((500, dim)).astype(np.float32)
    ix.upsert(np.arange(keep.size, keep.size + 500, dtype=np.int64), extra)
    both = np.vstack([new, stored(extra, dtype)])
    check(ix, both, dtype, np.ones(keep.size + 500, dtype=bool), q, 10, "appended after compaction")
    dist, rows = ix.search_scoped(q[:8], np.full(8, 2, dtype=np.uint32), 10)
    d_ref, r_ref = live_reference(both, dtype, np.flatnonzero(labels[keep] == 2), o.normalize_rows(q[:8]), 10)
    assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref), "the appended slots start without a label"
    ix.close()


@pytest.mark.parametrize("where", ["middle", "tail"])
def test_compact_below_a_pending_dirty_range_keeps_the_shadow_builds_inside_their_allocations(env, where):
    """Rows upserted since the last shadow build are a pending dirty range; compaction may shrink the count below its end.  The
    next shadow build must stop at the new count: the shadows are sized for the count (here still the ones allocated for 40,000
    rows + head room, 45,056), not for the old dirty range (up to row 60,000)."""
    _, Index, _ = env
    rng = np.random.default_rng(31 + len(where))
    n0, extra, dim, B = 40_000, 20_000, 768, 140
    raw = rng.standard_normal((n0 + extra, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n0, dtype=np.int64), raw[:n0])
    always_filter(ix)
    rows_ref = stored(raw, "f32")
    live = np.zeros(n0 + extra, dtype=bool)
    live[:n0] = True
    check(ix, rows_ref, "f32", live, q, 10, "int8 shadow built")
    ix.set_option("shadow8", 0)
    check(ix, rows_ref, "f32", live, q, 10, "2-byte shadow built")
    ix.set_option("shadow8", 1)
    assert ix.stat("shadow8_builds") == 1 and ix.stat("shadow16_builds") == 1
    ix.upsert(np.arange(n0, n0 + extra, dtype=np.int64), raw[n0:])          # past both shadows' head room, and no search: both dirty to 60,000
    live[n0:] = True
    if where == "middle":
        dead = np.concatenate([np.arange(10_000, 29_000), n0 + rng.permutation(extra)[:1500]])   # rows of the dirty range move down
    else:
        dead = np.concatenate([np.arange(n0 - 500, n0 + extra), rng.permutation(n0 - 500)[:300]])  # the whole dirty range goes
    ix.delete(dead)
    live[dead] = False
    keep = np.flatnonzero(live)
    assert ix.compact() == keep.size and keep.size <= 45_056
    new = ix.read_rows(0, keep.size)
    assert np.array_equal(new, rows_ref[keep])
    all_live = np.ones(keep.size, dtype=bool)
    check(ix, new, "f32", all_live, q, 10, "int8 path after compaction")
    assert ix.stat("shadow8_builds") == 2 and ix.stat("i8v2_passes") == 2
    ix.set_option("shadow8", 0)
    check(ix, new, "f32", all_live, q, 10, "2-byte path after compaction")
    assert ix.stat("shadow16_builds") == 2
    ix.set_option("shadow8", 1)
    # rows appended now land behind the compacted ones and are searched through both shadows
    more = rng.standard_normal((3000, dim)).astype(np.float32)
    ix.upsert(np.arange(keep.size, keep.size + 3000, dtype=np.int64), more)
    both = np.vstack([new, stored(more, "f32")])
    check(ix, both, "f32", np.ones(keep.size + 3000, dtype=bool), q, 10, "int8 path after append")
    ix.set_option("shadow8", 0)
    check(ix, both, "f32", np.ones(keep.size + 3000, dtype=bool), q, 10, "2-byte path after append")
    ix.close()


def test_compact_to_nothing_and_refill(env):
    _, Index, _ = env
    rng = np.random.default_rng(28)
    n, dim = 5000, 384
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    ix = Index(dim, dtype="f32")
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ix.delete(np.arange(n, dtype=np.int64))
    assert ix.compact() == 0 and ix.count() == 0
    dist, rows = ix.search(raw[:3], 5)
    assert (rows == -1).all() and np.isinf(dist).all()
    ix.upsert(np.arange(100, dtype=np.int64), raw[:100])
    check(ix, stored(raw[:100], "f32"), "f32", np.ones(100, dtype=bool), raw[:3], 5, "refilled")
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# an index that never saw a delete: the bits of the build before tombstones existed, for bench.py's seeded inputs
# (tests/golden/deletes_untouched_parent/*.npy were dumped by that build with the same command)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [256, 8])
def test_untouched_index_returns_the_bits_of_the_build_before_tombstones(tmp_path, batch):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "200000", "--batch", str(batch), "--steps", "2", "--warmup", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("distances.npy", "rows.npy"):
        got, want = np.load(os.path.join(out, name)), np.load(os.path.join(GOLDEN, f"b{batch}_{name}"))
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (batch, name)
