"""The input domain of the cosine on the GPU: tiny, huge and non-finite rows and queries on every search route.

Two references judge every answer.  The oracle (which restates canonical_norm literally) must be matched bit for bit: stored rows,
keys.  The fp64 cosine of the RAW inputs (tests/_cosine_reference.py: derivation of tol, the comparison rule and its 10 % cap) must be
matched within tol, so a defect the kernels and the oracle share cannot hide.  tests/test_input_domain.py holds the oracle to the
same reference on the CPU.

The corpus is the corpus() of test_gpu_global_rows.py (6,001 rows, exact ties) with about 5 % of its rows replaced by hostile ones.
On two-byte storage a random background cannot be ranked in fp64 within tol (the reference's docstring), so there the ordinary
queries, the planted row and the pair of equal rows are crafted to have ten decided neighbours."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _cosine_reference as ref
from tests._scoped_oracle_engine import ScopedOracleEngine
from tests.test_gpu_deletes import always_filter, expected_keys, stored
from tests.test_gpu_global_rows import ROUTES, Ctx, corpus, entry_points, row0_of, run
from tests.test_gpu_ivf_masked import K, N, NLIST, key_table, reference

pytestmark = pytest.mark.gpu

KINDS = ("2^-75", "2^-100", "2^63", "2^100", "4.47e-23", "subnormal", "nan", "+inf", "-inf", "zeros")
PICKS = 10


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import knn_index

    return torch, knn_index


def hostile_rows(rng, raw, keep):
    """about 5 % of the rows (none of `keep`) replaced, the ten kinds in turn; returns kind -> rows"""
    n, dim = raw.shape
    free = np.setdiff1d(np.arange(n), np.asarray(sorted(keep)))
    chosen = rng.choice(free, size=n // 20, replace=False)
    by_kind = {kind: chosen[i :: len(KINDS)] for i, kind in enumerate(KINDS)}
    for kind, rows in by_kind.items():
        for r in rows:
            v = rng.standard_normal(dim)
            if kind.startswith("2^"):
                raw[r] = np.ldexp(v, int(kind[2:])).astype(np.float32)
            elif kind == "4.47e-23":
                raw[r] = np.float32(4.47e-23)
            elif kind == "subnormal":
                raw[r] = np.ldexp(v, -135).astype(np.float32)           # every element below 2^-126 (a few round to zero)
                assert (np.abs(raw[r]) < 2.0**-126).all() and raw[r].any()
            elif kind == "zeros":
                raw[r] = 0.0
            else:
                raw[r] = v.astype(np.float32)
                raw[r, int(rng.integers(dim))] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    return by_kind


def hostile_case(rng, n, dim, B, dtype):
    """(raw, batches [L / B, B, dim], info): the hostile corpus and the queries of one route.

    The L queries (B, or the first multiple of B from 9 on), cut into batches of B: positions 0, 1, 2 hold a NaN query, a 2^-75 query and the tiny
    copy of the planted row; the middle two an inf query and a 2^100 query; the last three the query of the two equal rows (scaled
    by 2^-100), the huge copy of the planted row and a -inf query; from 40 queries on, position 3 is the query of the 40 equal rows."""
    raw, _, pair, clones = corpus(rng, n, dim, 2)
    keep = set(pair) | set(clones.tolist())
    by_kind = hostile_rows(rng, raw, keep)
    zero = np.flatnonzero(ref.is_zero_vector(raw))
    assert zero.size == sum(by_kind[kind].size for kind in ("nan", "+inf", "-inf", "zeros"))
    L = -(-max(9, B) // B) * B
    free = np.setdiff1d(np.arange(n), np.r_[sorted(keep), zero])
    planted = int(rng.choice(free))
    free = free[free != planted]
    t = ref.tol(dtype, o.pad_dim(dim))
    if dtype == "f32":                                                  # a random background is decided within 2 tol = 6e-6
        vec = rng.standard_normal((L + 2, dim)).astype(np.float32)
        vec[L], vec[L + 1] = raw[planted], raw[pair[0]]
    else:
        finite_hostile = np.concatenate([by_kind[kind] for kind in KINDS[:6]])
        distinct = np.concatenate([by_kind[kind] for kind in KINDS[:4] + KINDS[5:6]])   # (the constant rows are one direction: equal scores)
        picks = np.stack([np.r_[rng.choice(distinct, size=3, replace=False), rng.choice(np.setdiff1d(free, finite_hostile), size=PICKS - 3, replace=False)]
                          for _ in range(L + 2)])
        picks = rng.permuted(picks, axis=1)
        vec = ref.crafted_queries(raw, dtype, picks, t, floor=4.0 / np.sqrt(dim))
        raw[planted], raw[pair[0]], raw[pair[1]] = vec[L], vec[L + 1], vec[L + 1]
    q = vec[:L].copy()
    mid = L // 2
    q[0, dim // 3] = np.nan
    q[1] = np.ldexp(q[1], -75)
    q[2] = np.ldexp(raw[planted], -90)
    q[mid, 0] = np.inf
    q[mid + 1] = np.ldexp(q[mid + 1], 100)
    q[L - 3] = np.ldexp(raw[pair[0]], -100)
    q[L - 2] = np.ldexp(raw[planted], 90)
    q[L - 1, dim - 1] = -np.inf
    if B >= 40:
        q[3] = np.ldexp(raw[clones[0]], 64)
    info = Ctx()
    info.pair, info.clones, info.planted, info.by_kind, info.L, info.mid, info.zero_rows = pair, clones, planted, by_kind, L, mid, zero
    return raw, q.reshape(L // B, B, dim), info


def check_answer(keys, raw, q, dtype, info, k, what):
    """the keys of all L queries against both references; returns the left-out share"""
    dim = raw.shape[1]
    t = ref.tol(dtype, o.pad_dim(dim))
    rows_ref = stored(raw, dtype)
    keys0 = o.search_keys(rows_ref, dtype, o.normalize_rows(q), k, 0)
    bad = np.argwhere(keys != keys0)
    assert bad.size == 0, (what, f"{bad.shape[0]} keys differ from the oracle's, first {bad[0].tolist()}: {int(keys[tuple(bad[0])]):#018x} / {int(keys0[tuple(bad[0])]):#018x}")
    dist, rows = o.unpack_keys(keys)
    L, mid = info.L, info.mid
    # the copies of the planted row find it first, at distance 0 within tol; the equal rows lead their query, lower row first
    for b in (2, L - 2):
        assert rows[b, 0] == info.planted and abs(float(dist[b, 0])) <= t, (what, b, rows[b, 0], dist[b, 0])
    assert rows[L - 3, :2].tolist() == list(info.pair) and dist[L - 3, 0] == dist[L - 3, 1] and abs(float(dist[L - 3, 0])) <= t, what
    # no similarity above 1 + tol anywhere, and a hostile row that is the zero vector sits at distance exactly 1 wherever it shows up
    assert (dist[rows >= 0] >= -t).all(), (what, float(dist[rows >= 0].min()))
    assert (dist[np.isin(rows, info.zero_rows)] == 1.0).all(), what
    return ref.check(dist, rows, q, ref.scores64(q, raw, dtype), t, what=what, cap_ranks=PICKS if k > PICKS else None)


# ------------------------------------------------------------------------------------------------------------------------
# every unrestricted route
# ------------------------------------------------------------------------------------------------------------------------
MY_ROUTES = ROUTES + [("bf16_gemm_b300", "f32", 384, 6_001, 300, 10, True, {"shadow8": 0, "f16_tile": 0}, "filter_passes", False)]


@pytest.mark.parametrize("name,dtype,dim,n,B,k,forced,options,moved,at_sign", MY_ROUTES, ids=[r[0] for r in MY_ROUTES])
def test_every_route_answers_hostile_rows_and_queries(env, name, dtype, dim, n, B, k, forced, options, moved, at_sign):
    _, knn_index = env
    rng = np.random.default_rng(5200 + len(name) * 1000 + dim + B)
    raw, batches, info = hostile_case(rng, n, dim, B, dtype)
    ix = knn_index.DeviceKnnIndex(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    got, want = ix.read_rows(), stored(raw, dtype)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, "stored rows differ from the oracle's", np.flatnonzero((got != want).any(axis=1))[:8])
    assert ix.stat("all_normalized") == 1, "hostile rows must not cost the index its filters"
    if forced:
        always_filter(ix)
    for key, value in options.items():
        ix.set_option(key, value)
    keys = []
    for q in batches:
        before = ix.stat(moved)
        keys.append(ix.search_keys(q, k).cpu().numpy().view(np.uint64))
        assert ix.stat(moved) > before, (name, moved)
        # a non-finite query is the zero query, to itself and to its neighbours in the batch
        calm = np.where(np.isfinite(q).all(axis=1, keepdims=True), q, np.float32(0.0))
        assert np.array_equal(ix.search_keys(calm, k).cpu().numpy().view(np.uint64), keys[-1]), (name, "a non-finite query changed an answer")
    if name == "bf16_gemm_b300":
        assert ix.stat("filter_passes") >= 4, "300 queries go through two passes of at most 256"
    ix.close()
    check_answer(np.concatenate(keys), raw, batches.reshape(-1, dim), dtype, info, k, name)


# ------------------------------------------------------------------------------------------------------------------------
# the restricted routes, each once at dim 128, against the sub-matrix references the suite already has
# ------------------------------------------------------------------------------------------------------------------------
DIM, NPROBE, BMAX = 128, 8, 256


@pytest.fixture(scope="module")
def ctx(env):
    torch, knn_index = env
    c = Ctx()
    c.torch = torch
    rng = np.random.default_rng(5300)
    c.raw, batches, c.info = hostile_case(rng, N, DIM, BMAX, "f32")
    c.queries = batches[0]
    c.pair, c.clones = c.info.pair, c.info.clones
    c.rows_ref = stored(c.raw, "f32")
    qn = o.normalize_rows(c.queries)
    cent = rng.standard_normal((NLIST, DIM)).astype(np.float32)
    _, c.probed = o.search(o.normalize_rows(cent), "f32", qn, NLIST)
    c.assign = rng.choice(np.delete(np.arange(NLIST), 3), size=N, p=np.r_[0.3, 0.2, np.full(NLIST - 3, 0.5 / (NLIST - 3))])
    perm = np.argsort(c.assign, kind="stable").astype(np.int64)
    offsets = np.zeros(NLIST + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(c.assign, minlength=NLIST))
    c.labels = rng.integers(0, 5, N).astype(np.uint32)
    c.mask = rng.random(N) < 0.3
    hostile = np.concatenate(list(c.info.by_kind.values()))
    c.mask[hostile[::2]] = True                                # half of the hostile rows are allowed
    c.mask[[c.info.planted, *c.pair]] = True
    c.key_of = key_table(c.rows_ref, "f32", qn)
    c.lib = native.load()
    c.ix = knn_index.DeviceKnnIndex(DIM, dtype="f32")
    c.ix.upsert(np.arange(N, dtype=np.int64), c.raw)
    assert c.ix.read_rows().tobytes() == c.rows_ref.tobytes()
    c.ix.set_scopes(np.arange(N, dtype=np.int64), c.labels)
    t = [torch.from_numpy(a).to(c.ix.device) for a in (cent, perm, offsets)]
    native.check(c.lib.codd_knn_ivf_install(c.ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), c.ix._stream()), "codd_knn_ivf_install")
    c.oracle = ScopedOracleEngine(DIM, "f32")
    c.oracle.upsert(np.arange(N, dtype=np.int64), c.raw)
    c.oracle.set_scopes(np.arange(N, dtype=np.int64), c.labels)
    c.S = ref.scores64(c.queries, c.raw, "f32")
    yield c
    c.ix.close()


def check_restricted(c, call, keys0, B, what):
    """keys bit for bit against the sub-matrix reference; rows and distances are the unpacked keys; every distance is the fp64
    cosine of its row within tol; a zero query gets distance exactly 1 everywhere"""
    rc, keys, dist, rows = run(c, call, 0, B)
    assert rc == 0, (what, rc, native.last_error())
    bad = np.argwhere(keys != keys0)
    assert bad.size == 0, (what, f"{bad.shape[0]} keys differ, first {bad[0].tolist()}")
    d0, r0 = o.unpack_keys(keys0)
    assert np.array_equal(rows, r0) and np.array_equal(dist.view(np.uint32), d0.view(np.uint32)), what
    have = rows >= 0
    assert have.any() and np.isfinite(dist[have]).all(), what
    t = ref.tol("f32", DIM)
    err = np.abs((1.0 - dist.astype(np.float64)) - np.take_along_axis(c.S[:B], np.where(have, rows, 0), axis=1))[have]
    print(f"{what}: worst distance error {err.max():.3e} of tol {t:.3e} over {int(have.sum())} hits")
    assert err.max() <= t, (what, err.max())
    zero_q = ref.is_zero_vector(c.queries[:B])
    assert zero_q.any() and (dist[zero_q][have[zero_q]] == 1.0).all(), what


@pytest.mark.parametrize("B", (BMAX, 9))
def test_scoped_search_of_hostile_queries(ctx, B):
    c = ctx
    calls, scopes = entry_points(c, B)
    keys0 = c.oracle.search_keys_scoped(c.queries[:B], scopes, K, 0)
    before = c.ix.stat("scoped_searches")
    check_restricted(c, calls["search_scoped"], keys0, B, ("scoped", B))
    assert c.ix.stat("scoped_searches") == before + 1


@pytest.mark.parametrize("route,stat", [(1, "mask_list_searches"), (2, "mask_dense_searches")], ids=["list", "dense"])
def test_masked_search_of_hostile_queries(ctx, route, stat):
    c = ctx
    c.ix.set_option("mask_route", route)
    try:
        for B in (9, BMAX):
            calls, _ = entry_points(c, B)
            keys0 = expected_keys(c.rows_ref, "f32", c.mask, c.queries[:B], K, 0)
            for name in ("search_masked", "search_masked_dev"):
                before = c.ix.stat(stat)
                check_restricted(c, calls[name], keys0, B, (name, route, B))
                assert c.ix.stat(stat) == before + 1
            if B == BMAX:                       # the planted row and the equal rows are allowed: their scaled copies find them
                rows = row0_of(keys0)
                assert rows[2, 0] == c.info.planted and rows[BMAX - 2, 0] == c.info.planted and rows[BMAX - 3, :2].tolist() == list(c.pair)
    finally:
        c.ix.set_option("mask_route", 0)


@pytest.mark.parametrize("share,B", [(0, 9), (1, BMAX)], ids=["per_pair", "shared"])
def test_ivf_search_of_hostile_queries_plain_and_masked(ctx, share, B):
    c = ctx
    c.ix.set_option("ivf_share", share)
    try:
        calls, _ = entry_points(c, B)
        none_dead = np.zeros(N, dtype=bool)
        for name, mask in (("ivf_search", np.ones(N, dtype=bool)), ("ivf_search_masked", c.mask), ("ivf_search_masked_dev", c.mask)):
            keys0 = reference(c, B, NPROBE, mask, none_dead)
            before = c.ix.stat("ivf_shared_searches")
            check_restricted(c, calls[name], keys0, B, (name, share, B))
            assert c.ix.stat("ivf_shared_searches") == before + share, (name, share)
    finally:
        c.ix.set_option("ivf_share", 1)


# ------------------------------------------------------------------------------------------------------------------------
# normalize = 0: rows stored as they are, NaN and infinities included
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype", [(128, "f32"), (1536, "f32"), (1536, "f16")])
def test_rows_stored_as_they_are_rank_nan_scores_last(env, dim, dtype):
    _, knn_index = env
    n, k, B = 101, 128, 6                                       # k >= n: the whole ranking and the padding are visible
    rng = np.random.default_rng(5400 + dim)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    raw[5, 3] = np.nan
    raw[17, 0] = np.inf
    raw[40, dim - 1] = -np.inf
    raw[63, 7], raw[63, 9] = np.nan, np.inf
    raw[80] = 0.0
    raw[97, dim // 2], raw[97, dim // 2 + 1] = np.inf, -np.inf
    if dtype == "f16":
        raw[90, 11] = 70_000.0                                  # finite in fp32, infinite in f16
    q = rng.standard_normal((B, dim)).astype(np.float32)
    q[2] = 0.0                                                  # 0 * inf and 0 * NaN are NaN: the zero query meets them too
    q[4] = np.ldexp(q[4], -100)
    padded = np.zeros((n, o.pad_dim(dim)), dtype=np.float32)
    padded[:, :dim] = raw
    rows_ref = o.to_storage(padded, dtype)
    ix = knn_index.DeviceKnnIndex(dim, dtype=dtype)
    ix.upsert(np.arange(n, dtype=np.int64), raw, normalize=False)
    assert ix.stat("all_normalized") == 0
    assert np.array_equal(o.widen(ix.read_rows(), dtype), o.widen(rows_ref, dtype), equal_nan=True), "rows are stored as they are"
    if dtype == "f16":
        assert np.isinf(o.widen(ix.read_rows(), dtype)[90, 11])
    before = ix.stat("scan_launches")
    keys = ix.search_keys(q, k).cpu().numpy().view(np.uint64)
    dist, rows = ix.search(q, k)
    assert ix.stat("scan_launches") >= before + 2
    ix.close()
    keys0 = o.search_keys(rows_ref, dtype, o.normalize_rows(q), k, 0)
    assert np.array_equal(keys, keys0), np.argwhere(keys != keys0)[:4]
    d0, r0 = o.unpack_keys(keys0)
    assert np.array_equal(rows, r0) and np.array_equal(dist.view(np.uint32), d0.view(np.uint32))
    # the properties, from numpy alone: scores that are NaN (or -inf: the same key) come after every other, by lower row, at distance
    # +inf with their real row; the padding behind the n rows is -1 / +inf
    with np.errstate(invalid="ignore", over="ignore"):
        S = o.normalize_rows(q).astype(np.float64) @ o.widen(rows_ref, dtype).astype(np.float64).T
    last = np.isnan(S) | (S == -np.inf)
    assert last[:, [5, 63]].all() and last[2, [5, 17, 40, 63, 97]].all() and not last[:, 80].any()
    bound = (o.pad_dim(dim) / 64 + 7) * 2.0**-24 * np.sqrt((padded.astype(np.float64) ** 2)[np.isfinite(padded).all(axis=1)].sum(axis=1).max()) * 1.01
    for b in range(B):
        m = int(last[b].sum())
        assert rows[b, n - m : n].tolist() == np.flatnonzero(last[b]).tolist(), b
        assert (dist[b, n - m : n] == np.inf).all() and not np.isnan(dist[b]).any(), b
        assert np.sort(rows[b, :n]).tolist() == list(range(n)) and (rows[b, n:] == -1).all() and (dist[b, n:] == np.inf).all(), b
        head = dist[b, : n - m].astype(np.float64)            # scores of +inf first (distance -inf), then finite ones, ascending
        c = int((head == -np.inf).sum())
        assert (head[:c] == -np.inf).all() and np.isfinite(head[c:]).all() and (np.diff(head[c:]) >= 0).all(), b
        assert np.abs((1.0 - head[c:]) - S[b, rows[b, c : n - m]]).max() <= bound + 2.0**-24 * np.abs(head[c:]).max(), b
    assert (dist[2, : n - int(last[2].sum())] == 1.0).all()       # the zero query: +0 against every row that holds numbers


# ------------------------------------------------------------------------------------------------------------------------
# persistence
# ------------------------------------------------------------------------------------------------------------------------
def test_persist_reload_and_load_rows_keep_the_hostile_corpus(env, tmp_path):
    _, knn_index = env
    from codd_query_engine_amd import KnnClient

    n, dim, B, k = 2_001, 128, 16, 10
    rng = np.random.default_rng(5500)
    raw, batches, info = hostile_case(rng, n, dim, B, "f32")
    q = batches[0]
    ids = [f"r{i}" for i in range(n)]
    want_rows = stored(raw, "f32")
    d_ref, r_ref = o.search(want_rows, "f32", o.normalize_rows(q), k)

    def answers(col):
        got = col.query(query_embeddings=q, n_results=k, include=("distances",))
        return [[int(i[1:]) for i in row] for row in got["ids"]], np.asarray(got["distances"], dtype=np.float32)

    writer = KnnClient(path=str(tmp_path), device="cuda:0")
    col = writer.get_or_create_collection("hostile", metadata={"hnsw:space": "cosine"})
    col.upsert(ids=ids[:1500], embeddings=raw[:1500])
    assert writer.persist() == 1
    reader = KnnClient(path=str(tmp_path), device="cuda:0")
    assert reader.get_or_create_collection("hostile")._engine.read_rows().tobytes() == want_rows[:1500].tobytes()
    col.upsert(ids=ids[1500:], embeddings=raw[1500:])
    assert writer.persist() == 1 and reader.reload() == 1
    for who in (col, reader.get_or_create_collection("hostile")):
        assert who._engine.read_rows().tobytes() == want_rows.tobytes()
        assert who._engine.stat("all_normalized") == 1
        got_ids, got_dist = answers(who)
        assert got_ids == r_ref.tolist() and np.array_equal(got_dist.view(np.uint32), d_ref.view(np.uint32))
    ref.check(d_ref, r_ref, q, ref.scores64(q, raw, "f32"), ref.tol("f32", dim), what="persisted hostile corpus")
    # load_rows trusts nothing: its norm check must find every stored row a unit vector or a zero row, and keep the filters
    ix = knn_index.DeviceKnnIndex(dim)
    ix.load_rows(col._engine.read_rows())
    assert ix.stat("all_normalized") == 1 and ix.read_rows().tobytes() == want_rows.tobytes()
    dist, rows = ix.search(q, k)
    assert np.array_equal(rows, r_ref) and np.array_equal(dist.view(np.uint32), d_ref.view(np.uint32))
    ix.close()
