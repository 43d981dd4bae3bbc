"""ChromaDB's "l2" and "ip" spaces on the GPU: every answer — row ids AND the bits of every fp32 distance, or the
packed keys — must equal tests/_space_reference.py, the CPU restatement of the two canonical expressions.  No tolerance anywhere.

The shapes reach every instantiation the routing can launch: per storage dtype one width for each count of 16-byte chunks per lane
(NITER 1 .. 4) and a wide one (f32 384 and two-byte 1536 are there because they alone have NITER 2 and 3);
batches of 1, 4 and 5 .. 20 queries (the scan's groups of 1, 4 and 8, their remainders, several passes), k on both sides of 64 (one
and two list slots per lane), and for each of them the list scans of the scoped and the masked search."""

import ctypes

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _space_reference as sr

pytestmark = pytest.mark.gpu

N = 6001
SHAPES = [("f32", 70), ("f32", 200), ("f32", 384), ("f32", 768), ("f32", 1024), ("f32", 1536),
          ("bf16", 70), ("bf16", 768), ("bf16", 1536), ("bf16", 2048), ("bf16", 3072),
          ("f16", 70), ("f16", 768), ("f16", 1536), ("f16", 2048), ("f16", 3072)]
BATCHES = [(1, 1), (1, 128), (4, 10), (4, 100), (5, 10), (8, 128), (9, 10), (20, 100)]   # (B, k)
TOP = native.MAX_GLOBAL_ROW


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def inputs(n, d, B, seed):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = (1.3 * rng.standard_normal((B, d))).astype(np.float32)
    return raw, q


def build(Index, space, dtype, raw):
    ix = Index(raw.shape[1], dtype=dtype, space=space)
    ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw, normalize=False)
    return ix


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    (gd, gr), (wd, wr) = got, want
    gd, gr = np.asarray(gd), np.asarray(gr)
    assert np.array_equal(gr, wr), (what, "rows", np.flatnonzero((gr != wr).any(axis=1))[:8])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")


def keys_of(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("dtype,d", SHAPES)
def test_every_instantiation_equals_the_reference(Index, space, dtype, d):
    raw, q = inputs(N, d, 20, seed=d + len(dtype))
    q[3] = raw[17]                                        # a query equal to a stored row (before the storage rounding)
    ix = build(Index, space, dtype, raw)
    ref = sr.Reference(space, raw, dtype, q)
    assert np.array_equal(ix.read_rows(), ref.rows), "ingest differs from the reference"
    assert ix.stat("metric") == native.METRIC_CODES[space] and ix.stat("all_normalized") == 0
    for B, k in BATCHES:
        keys, dist, rows = ref.topk(B, k)
        same(ix.search(q[:B], k), (dist, rows), (space, dtype, d, B, k))
    # packed keys, the top global row at the 32-bit limit
    base = TOP - (N - 1)
    assert np.array_equal(keys_of(ix.search_keys(q[:5], 10, base)), ref.topk(5, 10, row_base=base)[0])
    # the list scans: scopes (1, 2, everything, nobody's) and a mask forced down the list route
    labels = np.zeros(N, dtype=np.uint32)
    labels[np.random.default_rng(d).permutation(N)[:900]] = np.repeat(np.array([1, 2], dtype=np.uint32), [37, 863])
    ix.set_scopes(np.arange(N, dtype=np.int64), labels)
    scopes = np.array([1, 2, 0, 99, 2], dtype=np.uint32)
    allow = np.random.default_rng(d + 1).random(N) < 0.3
    ix.set_option("mask_route", 1)
    for k in (10, 128):
        want = [ref.topk(1, k, allow=None if s == 0 else labels == s, queries=[b])[1:] for b, s in enumerate(scopes.tolist())]
        same(ix.search_scoped(q[:5], scopes, k), (np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])), (space, dtype, d, "scoped", k))
        same(ix.search_masked(q[:5], allow, k), ref.topk(5, k, allow=allow)[1:], (space, dtype, d, "masked", k))
    assert ix.stat("mask_list_searches") == 2 and ix.stat("filter_passes") == 0
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("dtype,d", [("f32", 70), ("f32", 1536), ("bf16", 768), ("f16", 3072)])
@pytest.mark.parametrize("n", [1, 3])
def test_fewer_rows_than_k_pads_with_minus_one_and_inf(Index, space, dtype, d, n):
    raw, q = inputs(n, d, 9, seed=n + d)
    ix = build(Index, space, dtype, raw)
    ref = sr.Reference(space, raw, dtype, q)
    for B, k in [(1, 1), (5, 10), (9, 128)]:
        keys, dist, rows = ref.topk(B, k)
        got_d, got_r = ix.search(q[:B], k)
        same((got_d, got_r), (dist, rows), (space, dtype, d, n, B, k))
        assert (got_r[:, min(n, k):] == -1).all() and np.isinf(got_d[:, min(n, k):]).all()
        got_k = keys_of(ix.search_keys(q[:B], k, 0))
        assert np.array_equal(got_k, keys) and (got_k[:, min(n, k):] == 0).all()
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_l2_values_that_only_the_direct_difference_gets_right(Index, dtype):
    """Unit-scale vectors, every element exactly representable in the storage dtype.  Rows 3 and 7 equal the query: distance bits
    0x00000000, the lower row first.  Row 5 differs in one element by 2^-12, row 2 by 2^-11: the differences and their squares
    are exact in fp32, so the distances are exactly 2^-24 and 2^-22.  |q|^2 + |c|^2 - 2<q, c> has 1 + 1 - 2 to cancel there."""
    d = 768
    rng = np.random.default_rng(9)
    u = rng.standard_normal(d)
    q = o.widen(o.to_storage((u / np.linalg.norm(u)).astype(np.float32)[None, :], dtype), dtype)[0]
    q[100] = q[200] = 2.0**-5                               # (2^-5 + 2^-12 and 2^-5 + 2^-11 are bf16 and fp16 numbers too)
    raw = (rng.standard_normal((40, d)) / np.sqrt(d)).astype(np.float32)
    raw[[3, 7, 5, 2]] = q
    raw[5, 100] += np.float32(2.0**-12)
    raw[2, 200] += np.float32(2.0**-11)
    ix = build(Index, "l2", dtype, raw)
    dist, rows = ix.search(q[None, :], 5)
    assert rows[0, :4].tolist() == [3, 7, 5, 2]
    assert bits(dist)[0, :4].tolist() == [0, 0, bits(np.float32(2.0**-24)).item(), bits(np.float32(2.0**-22)).item()]
    same((dist, rows), sr.Reference("l2", raw, dtype, q[None, :]).topk(1, 5)[1:], dtype)
    ix.close()


def test_ip_with_negative_scores_throughout(Index):
    rng = np.random.default_rng(4)
    raw = -np.abs(rng.standard_normal((500, 200))).astype(np.float32)
    q = np.abs(rng.standard_normal((5, 200))).astype(np.float32)
    ix = build(Index, "ip", "f32", raw)
    dist, rows = ix.search(q, 10)
    assert (dist > 1.0).all() and (np.diff(dist, axis=1) >= 0).all()
    same((dist, rows), sr.Reference("ip", raw, "f32", q).topk(5, 10)[1:], "negative ip")
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_zero_and_non_finite_vectors_are_the_zero_vector(Index, space, dtype):
    raw, q = inputs(300, 200, 6, seed=12)
    raw[3, 7], raw[9, 0], raw[20, 199], raw[30] = np.nan, np.inf, -np.inf, 0.0
    raw[31] = -0.0
    q[1, 5], q[2, 0], q[4] = np.nan, np.inf, 0.0
    ix = build(Index, space, dtype, raw)
    got = ix.read_rows()
    assert not got[[3, 9, 20, 30, 31]].any(), "zero and non-finite rows are stored as zeros (every bit clear)"
    ref = sr.Reference(space, raw, dtype, q)
    assert np.array_equal(got, ref.rows)
    dist, rows = ix.search(q, 10)
    same((dist, rows), ref.topk(6, 10)[1:], (space, dtype))
    if space == "ip":
        for b in (1, 2, 4):
            assert rows[b].tolist() == list(range(10)) and (dist[b] == 1.0).all(), "a zero query: rows 0 .. k-1 at distance exactly 1"
    else:
        sq = sr.l2_matrix(ref.rows, dtype, np.zeros((1, ref.rows.shape[1]), dtype=np.float32))[0]     # each row's canonical |c|^2
        for b in (1, 2, 4):
            assert np.array_equal(bits(dist[b]), bits(sq[rows[b]])) and dist[b, 0] == 0.0 and rows[b, 0] == 3
    # the device ingest stores the same bits
    import torch

    ix2 = Index(200, dtype=dtype, space=space)
    ix2.upsert_device(0, torch.from_numpy(raw).to("cuda:0"), normalize=False)
    torch.cuda.synchronize()
    assert np.array_equal(ix2.read_rows(), got)
    ix.close()
    ix2.close()


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("dtype,d", [("f32", 200), ("bf16", 768), ("f16", 3072)])
def test_every_route(Index, space, dtype, d):
    import torch

    from codd_query_engine_amd import knn_index

    B, k = 9, 10
    raw, q = inputs(N, d, B, seed=d)
    raw[4000] = raw[10]                                    # duplicate rows, one in each shard below
    q[0] = raw[10]
    ix = build(Index, space, dtype, raw)
    ref = sr.Reference(space, raw, dtype, q)
    want_keys, want_d, want_r = ref.topk(B, k)
    same(ix.search(q, k), (want_d, want_r), "flat")
    if space == "l2":
        assert want_r[0, :2].tolist() == [10, 4000], "duplicates: the lower row first"
    # two shards' keys through merge_shards / merge_keys, with the space, equal the flat search
    cut = 3000
    a, b = build(Index, space, dtype, raw[:cut]), build(Index, space, dtype, raw[cut:])
    ka, kb = a.search_keys(q, k, 0), b.search_keys(q, k, cut)
    mk, md, mr = knn_index.merge_shards(torch.cat([ka, kb]), 2, k, space=space)
    assert np.array_equal(keys_of(mk), want_keys)
    same((md.cpu().numpy(), mr.cpu().numpy()), (want_d, want_r), "merge_shards")
    mk, md, mr = a.merge_keys(torch.cat([ka, kb], dim=1), k)
    assert np.array_equal(keys_of(mk), want_keys)
    same((md.cpu().numpy(), mr.cpu().numpy()), (want_d, want_r), "merge_keys")
    a.close()
    b.close()
    # masks: host words and device words, both routes, and a mask that allows nothing
    allow = np.random.default_rng(d).random(N) < 0.4
    words = np.zeros((N + 31) // 32 * 4, dtype=np.uint8)
    packed = np.packbits(allow, bitorder="little")
    words[: packed.shape[0]] = packed
    dev_words = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    want = ref.topk(B, k, allow=allow)[1:]
    for route in (1, 2):
        ix.set_option("mask_route", route)
        same(ix.search_masked(q, allow, k), want, ("host mask", route))
        same(ix.search_masked_dev(q, dev_words, k), want, ("device mask", route))
        base = TOP - (N - 1)
        assert np.array_equal(keys_of(ix.search_keys_masked(q, allow, k, base)), ref.topk(B, k, allow=allow, row_base=base)[0])
        none_d, none_r = ix.search_masked(q, np.zeros(N, dtype=bool), k)
        assert (none_r == -1).all() and np.isinf(none_d).all()
    assert ix.stat("mask_list_searches") == 3 and ix.stat("mask_dense_searches") == 3
    ix.set_option("mask_route", 0)
    # deletes, then compact: the same answers on the renumbered rows
    gone = np.unique(np.concatenate([want_r[:, :3].ravel(), np.arange(100, 400)]))
    live = np.ones(N, dtype=bool)
    live[gone] = False
    ix.delete(gone)
    w_d, w_r = ref.topk(B, k, allow=live)[1:]
    same(ix.search(q, k), (w_d, w_r), "after delete")
    same(ix.search_masked(q, allow, k), ref.topk(B, k, allow=allow & live)[1:], "mask after delete")
    assert ix.compact() == int(live.sum())
    new_slot = np.cumsum(live) - 1
    same(ix.search(q, k), (w_d, np.where(w_r >= 0, new_slot[np.where(w_r >= 0, w_r, 0)], -1)), "after compact")
    # upsert overwrite, upsert_device, and load_rows of read_rows' output
    kept = raw[live].copy()
    kept[[5, 77]] = raw[gone[:2]]
    ix.upsert(np.array([5, 77], dtype=np.int64), kept[[5, 77]], normalize=False)
    extra = (1.1 * np.random.default_rng(1).standard_normal((64, d))).astype(np.float32)
    ix.upsert_device(kept.shape[0], torch.from_numpy(extra).to("cuda:0"), normalize=False)
    kept = np.concatenate([kept, extra])
    ref2 = sr.Reference(space, kept, dtype, q)
    same(ix.search(q, k), ref2.topk(B, k)[1:], "after overwrite and device upsert")
    stored = ix.read_rows()
    assert np.array_equal(stored, ref2.rows)
    loaded = Index(d, dtype=dtype, space=space)
    loaded.load_rows(stored)
    assert np.array_equal(loaded.read_rows(), stored) and loaded.stat("all_normalized") == 0
    same(loaded.search(q, k), ref2.topk(B, k)[1:], "loaded rows")
    ix.close()
    loaded.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_no_filter_leg_whatever_the_batch(Index, space):
    raw, q = inputs(N, 200, 256, seed=2)
    ix = build(Index, space, "f32", raw)
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)                              # what sends a cosine index of this size to the filters
    ref = sr.Reference(space, raw, "f32", q[:20])
    same(ix.search(q[:20], 10), ref.topk(20, 10)[1:], "B = 20")
    dist, rows = ix.search(q, 10)
    same((dist[:20], rows[:20]), ref.topk(20, 10)[1:], "B = 256, its first 20 queries")
    assert ix.stat("last_scan_group") == 8 and ix.stat("scan_launches") == 2
    for key in ("filter_passes", "shadow8_builds", "shadow16_builds", "shadow8_passes", "i8v2_passes"):
        assert ix.stat(key) == 0, key
    assert ix.stat("metric") == native.METRIC_CODES[space]
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_ivf_and_approx_scores_refuse(Index, space):
    import torch

    from codd_query_engine_amd import ivf

    raw, q = inputs(2000, 64, 4, seed=6)
    ix = build(Index, space, "f32", raw)
    lib = native.load()
    dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    qd, cent = dev(q), dev(raw[:8].copy())
    perm, offs = dev(np.arange(2000, dtype=np.int64)), dev(np.linspace(0, 2000, 9).astype(np.int64))
    out_d, out_r = torch.empty((4, 5), device="cuda:0"), torch.empty((4, 5), dtype=torch.int64, device="cuda:0")
    scores = torch.empty((256, 2000), device="cuda:0")
    before = (ix.stat("searches"), ix.stat("scan_launches"), native.live_allocations())
    assert lib.codd_knn_ivf_install(ix._h, cent.data_ptr(), 8, perm.data_ptr(), offs.data_ptr(), None) == -95
    assert "cosine" in native.last_error()
    assert lib.codd_knn_ivf_search(ix._h, qd.data_ptr(), 4, 5, 2, 0, None, out_d.data_ptr(), out_r.data_ptr(), None) == -95
    assert lib.codd_knn_approx_scores(ix._h, qd.data_ptr(), 4, scores.data_ptr(), None) == -95
    assert (ix.stat("searches"), ix.stat("scan_launches"), native.live_allocations()) == before, "a refusal enqueues and allocates nothing"
    for call in (lambda: ivf.build_ivf(ix, 8), lambda: ivf.search_ivf(ix, q, 5, 2), lambda: ivf.search_ivf_keys(ix, q, 5, 2),
                 lambda: ivf.IvfShardEngine(ix, 2), lambda: ix.approx_scores(q)):
        with pytest.raises(native.NativeLibraryError, match="cosine"):
            call()
    ix.close()


def test_cosine_is_untouched(Index):
    raw, q = inputs(N, 768, 9, seed=8)
    ix = Index(768, dtype="f32")
    assert ix.space == "cosine" and ix.stat("metric") == 0 and ix.stat("all_normalized") == 1
    ix.upsert(np.arange(N, dtype=np.int64), raw)
    rows_ref = o.normalize_rows(raw)
    assert np.array_equal(ix.read_rows(), rows_ref)
    for B, k in [(1, 10), (4, 100), (9, 10)]:
        d_ref, r_ref = o.search(rows_ref, "f32", o.normalize_rows(q[:B]), k)
        same(ix.search(q[:B], k), (d_ref, r_ref), ("cosine", B, k))
    ix.close()
