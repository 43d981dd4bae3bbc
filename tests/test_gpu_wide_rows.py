"""Rows wider than the register-resident kernels take: f32 rows of 1,025 .. 4,096 elements, bf16 / fp16 rows of 2,049 .. 4,096
(1,536 and 3,072: the OpenAI embedders; 4,096: LLM-based ones).  Every exact score on these rows comes from the wide forms of the
scan, finalize, anchor and IVF kernels (the row walked in segments, each lane's fmaf chain carried across them), so every answer
must equal the oracle's bit for bit, rows and fp32 distances, and the stats must show which path ran."""

import ctypes

import numpy as np
import pytest

from oracle import knn_oracle as o

pytestmark = pytest.mark.gpu

FILTER_KEYS = ("filter_min_rows", "filter_min_rows_small", "filter_min_batch")


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def corpus(n, d, B, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    q[0] = raw[n // 3]                                                            # a query equal to a stored row
    if B > 1:
        q[1] = raw[n - 1] + 0.05 * rng.standard_normal(d).astype(np.float32)      # its neighbour in the ragged last tile
    return raw, q


def make(Index, raw, dtype, filtered=False, shadow8=1):
    ix = Index(raw.shape[1], dtype=dtype)
    ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw)
    if filtered:
        for key in FILTER_KEYS:
            ix.set_option(key, 1)
        ix.set_option("shadow8", shadow8)
    else:
        ix.set_option("filter", 0)
    return ix


def oracle_answer(raw, q, k, dtype):
    return o.search(o.to_storage(o.normalize_rows(raw), dtype), dtype, o.normalize_rows(q), k)


def assert_exact(ix, raw, q, k, dtype, reps=1):
    d_ref, i_ref = oracle_answer(raw, q, k, dtype)
    for rep in range(reps):
        dist, rows = ix.search(q, k)
        assert np.array_equal(rows, i_ref), rep
        assert np.array_equal(dist, d_ref), rep


WIDTHS = [(1025, "f32"), (1536, "f32"), (2048, "f32"), (3072, "f32"), (4095, "f32"), (4096, "f32"),
          (2049, "bf16"), (3072, "bf16"), (4096, "bf16"), (2049, "f16"), (3072, "f16"), (4096, "f16")]


@pytest.mark.parametrize("d,dtype", WIDTHS)
def test_exact_scan(Index, d, dtype):
    """filter = 0: scan_topk_wide_kernel with 1, 4 and 8 queries per pass over the rows, one and two list slots."""
    n = 6_001
    raw, q = corpus(n, d, 1024, d)
    ix = make(Index, raw, dtype)
    scans = 0
    for B in (1, 8, 1024):
        for k in (10, 100):
            assert_exact(ix, raw, q[:B], k, dtype)
            scans += 1
            # queries per pass over the rows: 8 over f32 rows, at most 4 over 2-byte rows
            assert ix.stat("last_scan_group") == (1 if B == 1 else (8 if dtype == "f32" else 4))
    assert ix.stat("scan_launches") >= scans and ix.stat("filter_passes") == 0
    ix.close()


@pytest.mark.parametrize("d,dtype", WIDTHS)
@pytest.mark.parametrize("B", [1, 32, 100, 256])
def test_int8_filter(Index, d, dtype, B):
    """The int8 shadow (built in column slices above 2,048 elements), its thresholds (anchor_thr_kernel's wide form) and the
    exact re-score of the survivors (finalize's wide form; B = 1 shares each query out over 16 workgroups).  B = 100 runs the
    tile program's 8-query blocks, B = 256 its 16-query blocks.  Searched twice: the same bits both times."""
    n = 10_000
    raw, q = corpus(n, d, B, d + B)
    ix = make(Index, raw, dtype, filtered=True)
    assert_exact(ix, raw, q, 10, dtype, reps=2)
    assert ix.stat("shadow8_passes") == 2 and ix.stat("fallback_queries") == 0
    assert ix.stat("last_finalize_parts") == {1: 16, 32: 8, 100: 1, 256: 1}[B]
    if B >= 65:
        assert ix.stat("i8v2_passes") == 2
    # the block-scaled int8 error norm of a Gaussian unit row stays far below the 0.04 cut-off at every width
    assert 0 < ix.stat("shadow8_eps_r_micro") < 20_000 and ix.stat("shadow8_wide_blocks") == 0
    ix.close()


@pytest.mark.parametrize("d,dtype,B,tile", [(1536, "f32", 256, True), (3072, "bf16", 256, True), (3072, "f16", 129, True),
                                            (4096, "f32", 256, False), (4096, "bf16", 32, False), (2049, "f16", 100, False)])
def test_two_byte_filter(Index, d, dtype, B, tile):
    """shadow8 = 0: the fp16 MFMA filter; at 24 and 48 K-steps of 64 (1,536 / 3,072 elements) its tile program."""
    n = 15_000
    raw, q = corpus(n, d, B, 7 * d + B)
    ix = make(Index, raw, dtype, filtered=True, shadow8=0)
    assert_exact(ix, raw, q, 10, dtype, reps=2)
    assert ix.stat("filter_passes") == 2 and ix.stat("shadow8_passes") == 0 and ix.stat("fallback_queries") == 0
    assert (ix.stat("f16_tile_passes") == 2) == tile
    ix.close()


@pytest.mark.parametrize("d,dtype,B,k,n", [(4096, "f32", 256, 10, 10_000), (3072, "bf16", 32, 10, 10_000), (1536, "f32", 100, 100, 120_000),
                                             (4096, "f16", 1, 10, 10_000)])
def test_forced_fallback_is_exact(Index, d, dtype, B, k, n):
    """A candidate list capped far below what the queries leave: every query goes to the list-driven wide exact scan (k = 100:
    enough rows that the thresholds have twice k sampled tiles, else the search is an exact scan from the start)."""
    raw, q = corpus(n, d, B, 11 * d + B)
    ix = make(Index, raw, dtype, filtered=True)
    ix.set_option("hit_cap", 16)
    assert_exact(ix, raw, q, k, dtype)
    assert ix.stat("fallback_queries") > 0
    ix.close()


@pytest.mark.parametrize("d,dtype", [(4096, "f32"), (3072, "bf16"), (2049, "f16")])
@pytest.mark.parametrize("filtered", [False, True])
def test_special_rows(Index, d, dtype, filtered):
    """Zero rows (stored as zeros, score 0), exact and near duplicates (ties: lower row first), a zero query, a query equal to a
    stored row and one whose neighbours sit in the ragged last tile."""
    n = 9_001
    rng = np.random.default_rng(d)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    raw[100:110] = 0.0
    raw[200:210] = raw[50]                                                     # exact duplicates of row 50
    raw[300:310] = raw[60] + 1e-4 * rng.standard_normal((10, d)).astype(np.float32)   # near duplicates of row 60
    raw[n - 5:] = raw[70] + 1e-3 * rng.standard_normal((5, d)).astype(np.float32)     # ... of row 70, in the last tile
    q = rng.standard_normal((40, d)).astype(np.float32)
    q[0], q[1], q[2], q[3] = raw[50], raw[60], raw[70], 0.0
    ix = make(Index, raw, dtype, filtered=filtered)
    for k in (10, 100):
        assert_exact(ix, raw, q, k, dtype)
    _, rows = ix.search(q[:3], 10)
    assert list(rows[0]) == [50] + list(range(200, 209))
    ix.close()


def test_ivf_exhaustive_probe_equals_flat_search_at_3072(Index):
    """ivf_scan_kernel (few pairs) and ivf_scan_shared_kernel (>= 1,024 pairs) in their wide forms: nprobe == nlist is the flat search."""
    import torch

    from codd_query_engine_amd import ivf

    n, d, nlist = 12_000, 3072, 16
    raw, _ = corpus(n, d, 1, 5)
    ix = Index(d, "f32")
    ix.upsert_device(0, torch.from_numpy(raw).cuda().contiguous())
    ivf.build_ivf(ix, nlist, iters=3)
    q = torch.from_numpy(np.random.default_rng(6).standard_normal((64, d)).astype(np.float32)).cuda()
    for B, k in ((9, 10), (9, 100), (64, 10), (64, 100)):
        d_flat, r_flat = ix.search_tensors(q[:B], k)
        shared = ix.stat("ivf_shared_searches")
        d_ivf, r_ivf = ivf.search_ivf(ix, q[:B], k, nprobe=nlist)
        assert torch.equal(r_ivf, r_flat) and torch.equal(d_ivf, d_flat), (B, k)
        # 64 x 16 = 1,024 (query, list) pairs: each probed list scanned once for its queries; 9 x 16: once per pair
        assert ix.stat("ivf_shared_searches") - shared == (1 if B == 64 else 0), (B, k)
    ix.close()


@pytest.mark.parametrize("dtype,B", [("f32", 8), ("bf16", 256)])
def test_sharded_halves_merge_to_the_whole(Index, dtype, B):
    import torch

    from codd_query_engine_amd.knn_index import merge_shards

    n, d, cut = 10_000, 4096, 4_321
    raw, q = corpus(n, d, B, 9)
    whole = make(Index, raw, dtype, filtered=True)
    s0, s1 = make(Index, raw[:cut], dtype, filtered=True), make(Index, raw[cut:], dtype, filtered=True)
    d_ref, i_ref = oracle_answer(raw, q, 10, dtype)
    gathered = torch.cat([s0.search_keys(q, 10, 0), s1.search_keys(q, 10, cut)], dim=0)
    _, d2, i2 = merge_shards(gathered, 2, 10)
    assert np.array_equal(i2.cpu().numpy(), i_ref) and np.array_equal(d2.cpu().numpy(), d_ref)
    dist, rows = whole.search(q, 10)
    assert np.array_equal(rows, i_ref) and np.array_equal(dist, d_ref)
    for ix in (whole, s0, s1):
        ix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_storage_round_trips_at_4096(Index, dtype):
    """upsert_device writes what upsert writes; read_rows -> load_rows gives back an index that searches the same."""
    import torch

    n, d = 5_000, 4096
    raw, q = corpus(n, d, 40, 13)
    a = Index(d, dtype)
    a.upsert_device(0, torch.from_numpy(raw).cuda().contiguous())
    stored = a.read_rows()
    assert np.array_equal(stored, o.to_storage(o.normalize_rows(raw), dtype))
    b = Index(d, dtype)
    b.load_rows(stored)
    assert b.stat("all_normalized") == 1
    assert np.array_equal(b.read_rows(), stored)
    for ix in (a, b):
        for key in FILTER_KEYS:
            ix.set_option(key, 1)
        assert_exact(ix, raw, q, 10, dtype)
    a.close()
    b.close()


def test_client_persist_and_reload_at_4096(tmp_path):
    from codd_query_engine_amd import HashingEmbeddingFunction, KnnClient

    emb = HashingEmbeddingFunction(4096)
    docs = [f"metric {i} latency of service {i % 7} in region {i % 5}" for i in range(300)]
    writer = KnnClient(device="cuda:0", path=str(tmp_path), embedding_function=emb)
    col = writer.get_or_create_collection("wide")
    col.upsert(ids=[f"m{i}" for i in range(len(docs))], documents=docs)
    before = col.query(query_texts=["latency of service 3", "region 4"], n_results=20)
    rows_before = col._engine.read_rows()
    assert writer.persist() == 1
    reader = KnnClient(device="cuda:0", path=str(tmp_path), embedding_function=emb)
    rcol = reader.get_collection("wide")
    assert rcol.count() == len(docs) and np.array_equal(rcol._engine.read_rows(), rows_before)
    assert rcol.query(query_texts=["latency of service 3", "region 4"], n_results=20) == before


def test_store_over_wide_embedder_matches_the_checker_engine():
    """MetricsSemanticMetadataStore over a KnnClient whose embedder returns 1,536-wide vectors answers as over the CPU oracle."""
    from codd_query_engine_amd import HashingEmbeddingFunction, KnnClient, MetricsSemanticMetadataStore
    from tests._oracle_engine import OracleEngine

    emb = HashingEmbeddingFunction(1536)
    stores = [MetricsSemanticMetadataStore(KnnClient(device="cuda:0", embedding_function=emb)),
              MetricsSemanticMetadataStore(KnnClient(engine_factory=lambda dim: OracleEngine(dim), embedding_function=emb))]
    records = [{"metric_name": f"svc{i}.{kind}", "description": f"{kind} of service {i} measured per {unit}", "category": kind}
               for i in range(40) for kind, unit in (("latency", "request"), ("throughput", "second"), ("errors", "minute"))]
    for s in stores:
        s.index_metadata_batch("ns", records)
    for query in ("latency of service 7", "errors per minute", "throughput"):
        a, b = (s.search_metadata(query, n_results=15) for s in stores)
        assert a == b, query


def test_cabi_create_accepts_4096_and_refuses_4097(Index):
    from codd_query_engine_amd import native

    lib = native.load()
    for dtype in (0, 1, 2):
        h = ctypes.c_void_p()
        assert lib.codd_knn_create(ctypes.byref(h), 0, 4096, dtype, 0) == 0, native.last_error()
        assert lib.codd_knn_destroy(h) == 0
        assert lib.codd_knn_create(ctypes.byref(h), 0, 4097, dtype, 0) == -22
