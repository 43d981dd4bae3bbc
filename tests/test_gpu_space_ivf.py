"""IVF on an ip or l2 index (option "space_ivf"): the coarse index, the list scans and the build in the index's own
space.  The contract is the cosine one: the exact canonical top-k among the allowed live rows of the nprobe probed lists, and an
exhaustive probe is the flat search bit for bit.

Most tests install a layout they made themselves (codd_knn_ivf_install takes any centroids, permutation and offsets), so they know
every list's rows and no k-means is involved.  The expected answer comes from tests/_space_reference.py alone: the probes are the
reference's top-nprobe over the centroids (an f32 index of the same space), the answer its top-k over the rows of those lists.
Keys, the bits of every distance and the rows are compared; no tolerance anywhere."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _space_reference as sr

pytestmark = pytest.mark.gpu

ROW_BASE = 1_000


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex, ivf


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def keys_of(t):
    return t.cpu().numpy().view(np.uint64)


def words_of(mask):
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((mask.shape[0] + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    return words.view("<u4").copy()


def lists_of(n, nlist):
    """list(row) = (7 row + 3) mod nlist; list nlist - 2 emptied into list 0; list nlist - 1 keeps its first row, the others go to
    list 1.  -> (assign, perm: the stable sort by list, offsets)"""
    assign = (7 * np.arange(n) + 3) % nlist
    assign[assign == nlist - 2] = 0
    last = np.flatnonzero(assign == nlist - 1)
    assign[last[1:]] = 1
    sizes = np.bincount(assign, minlength=nlist)
    assert sizes[nlist - 2] == 0 and sizes[nlist - 1] == 1 and all(s % 16 for s in sizes if s), sizes
    perm = np.argsort(assign, kind="stable").astype(np.int64)
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes)
    return assign, perm, offsets


class Case:
    """One hand-installed layout of one space: the index, the reference over its rows, the probes of every query."""

    def __init__(self, env, space, n, d, dtype, nlist, B, seed, option=1, repeat_half=False):
        torch, Index, _ = env
        self.torch, self.space, self.n, self.nlist, self.dtype = torch, space, n, nlist, dtype
        rng = np.random.default_rng(seed)
        self.raw = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
        cent = rng.standard_normal((nlist, d))
        self.cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (nlist, 1))).astype(np.float32)
        self.assign, self.perm, self.offsets = lists_of(n, nlist)
        q = (1.3 * rng.standard_normal((B, d))).astype(np.float32)
        q[1] = 0.0                                            # a zero query
        q[2, 5 % d] = np.nan                                  # a query with a NaN element: the zero vector
        # a query equal to a stored row, as stored: the first row whose own list is among the lists that row probes at nprobe 4
        st = sr.stored(self.raw, dtype)
        as_stored = o.widen(st[:64], dtype)[:, :d].copy()
        near = sr.Reference(space, self.cent, "f32", as_stored).topk(64, 4)[2]
        self.twin = int(np.flatnonzero((near == self.assign[:64, None]).any(axis=1))[0])
        q[3] = as_stored[self.twin]
        self.nuniq = B
        if repeat_half:                                       # half of the batch is one query: one list, many pairs
            q[B // 2:] = q[0]
            self.nuniq = B // 2
        self.q = q
        self.ref = sr.Reference(space, self.raw, dtype, q[: self.nuniq], rows_storage=st)
        self.cref = sr.Reference(space, self.cent, "f32", q[: self.nuniq])
        self.ix = Index(d, dtype=dtype, space=space)
        self.ix.set_option("space_ivf", option)
        self.ix.upsert(np.arange(n, dtype=np.int64), self.raw, normalize=False)
        self.dead = np.zeros(n, dtype=bool)

    def install(self, ix=None):
        ix = ix or self.ix
        t = [self.torch.from_numpy(a).to(ix.device) for a in (self.cent, self.perm, self.offsets)]
        return native.load().codd_knn_ivf_install(ix._h, t[0].data_ptr(), self.nlist, t[1].data_ptr(), t[2].data_ptr(), ix._stream())

    def expected(self, B, k, nprobe, mask=None, row_base=0):
        """(keys, dist, rows) [B, k]: per query the reference's top-k among the allowed live rows of the lists the reference probes"""
        probes = self.cref.topk(self.nuniq, min(nprobe, self.nlist))[2]
        allowed = ~self.dead if mask is None else (mask & ~self.dead)
        out = []
        for b in range(B):
            u = b if b < self.nuniq else 0
            allow = np.isin(self.assign, probes[u]) & allowed
            out.append(self.ref.topk(1, k, allow=allow, row_base=row_base, queries=[u]))
        return tuple(np.concatenate([x[i] for x in out]) for i in range(3))

    def check(self, ivf, B, k, nprobe, mask=None, what=None):
        """search_ivf (distances, rows) and search_ivf_keys under a row base against the reference; -> the keys"""
        keys, dist, rows = self.expected(B, k, nprobe, mask, row_base=ROW_BASE)
        gd, gr = ivf.search_ivf(self.ix, self.q[:B], k, nprobe, allow=mask)
        gd, gr = gd.cpu().numpy(), gr.cpu().numpy()
        assert np.array_equal(gr, rows), (what, "rows", np.flatnonzero((gr != rows).any(axis=1))[:8])
        assert np.array_equal(bits(gd), bits(dist)), (what, "distance bits")
        gk = keys_of(ivf.search_ivf_keys(self.ix, self.q[:B], k, nprobe, ROW_BASE, allow=mask))
        assert np.array_equal(gk, keys), (what, "keys", np.flatnonzero((gk != keys).any(axis=1))[:8])
        return gk


FORMS = [
    (3_000, 100, "f32", 24, 9, 5, 10),     # ragged width, fewer chunks than lanes
    (3_000, 768, "f32", 24, 9, 5, 100),    # NITER 3, two list slots
    (3_000, 1_024, "f16", 24, 9, 5, 10),   # NITER 2, 2-byte widening
    (2_000, 2_048, "bf16", 16, 9, 5, 10),  # 2-byte NITER 4: never the shared scan
    (2_000, 1_536, "f32", 16, 5, 4, 10),   # the wide form
]


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("n,d,dtype,nlist,B,nprobe,k", FORMS, ids=[f"{f[1]}-{f[2]}" for f in FORMS])
def test_each_row_form_equals_the_reference(env, space, n, d, dtype, nlist, B, nprobe, k):
    _, _, ivf = env
    c = Case(env, space, n, d, dtype, nlist, B, seed=d + len(dtype))
    try:
        assert c.ix.stat("space_ivf") == 1 and c.install() == 0, native.last_error()
        assert np.array_equal(c.ix.read_rows(), c.ref.rows)
        c.check(ivf, B, k, nprobe, what=(space, d, dtype))
        c.check(ivf, 1, k, nprobe, what=(space, d, dtype, "B=1"))
        gd, gr = ivf.search_ivf(c.ix, c.q[:B], k, nprobe)
        gd, gr = gd.cpu().numpy(), gr.cpu().numpy()
        # the zero query and the NaN query are the same query
        assert np.array_equal(gr[1], gr[2]) and np.array_equal(bits(gd[1]), bits(gd[2]))
        if space == "l2":   # the query equal to a stored row of a probed list: distance +0.0, first
            assert gr[3, 0] == c.twin and bits(gd[3, 0]) == 0, (gr[3, :3], gd[3, :3])
            assert (gd[gr >= 0] >= 0).all()
    finally:
        c.ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("n,d,dtype,nlist", [(4_000, 128, "f32", 32), (4_000, 128, "f16", 32), (2_000, 1_536, "f32", 16)],
                         ids=["128-f32", "128-f16", "1536-f32"])
def test_the_shared_scan_returns_the_per_pair_scan_s_bits_and_the_reference_s(env, space, n, d, dtype, nlist):
    _, _, ivf = env
    B, nprobe, k = 64, 16, 10                 # 1,024 pairs >= 2 nlist: the list-sharing scan
    c = Case(env, space, n, d, dtype, nlist, B, seed=31 + d, repeat_half=True)
    try:
        assert c.install() == 0, native.last_error()
        want = c.expected(B, k, nprobe, row_base=ROW_BASE)[0]
        c.ix.set_option("ivf_share", 0)
        before = c.ix.stat("ivf_shared_searches")
        k0 = keys_of(ivf.search_ivf_keys(c.ix, c.q, k, nprobe, ROW_BASE))
        assert c.ix.stat("ivf_shared_searches") == before
        c.ix.set_option("ivf_share", 1)
        k1 = keys_of(ivf.search_ivf_keys(c.ix, c.q, k, nprobe, ROW_BASE))
        assert c.ix.stat("ivf_shared_searches") == before + 1
        k2 = keys_of(ivf.search_ivf_keys(c.ix, c.q, k, nprobe, ROW_BASE))   # the grouping scratch is reused
        assert np.array_equal(k0, want), np.flatnonzero((k0 != want).any(axis=1))[:8]
        assert np.array_equal(k1, k0) and np.array_equal(k2, k0)
        c.check(ivf, B, k, nprobe, what=(space, d, dtype, "shared"))          # ... and the distances and rows written behind it
    finally:
        c.ix.close()


def clustered(rng, centres, n, d):
    return (centres[rng.integers(0, centres.shape[0], n)] + 0.5 * rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)


def corpus(n, d, ncentres, nq, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((ncentres, d))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (ncentres, 1))
    return clustered(rng, c, n, d), clustered(rng, c, nq, d)


@pytest.mark.parametrize("space", sr.SPACES)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_exhaustive_probe_is_the_flat_search(env, space, dtype):
    torch, Index, ivf = env
    n, d, nlist = 6_000, 128, 16
    x, q = corpus(n, d, 32, 9, seed=5)
    q[1] = 0.0
    q[3] = x[17]
    ix = Index(d, dtype=dtype, space=space)
    ix.set_option("space_ivf", 1)
    ix.upsert(np.arange(n, dtype=np.int64), x, normalize=False)
    stats = ivf.build_ivf(ix, nlist, iters=3)
    assert stats["rows"] == n
    qd = torch.from_numpy(q).to(ix.device)
    for k in (1, 10, 100):
        d_flat, r_flat = ix.search_tensors(qd, k)
        d_ivf, r_ivf = ivf.search_ivf(ix, qd, k, nprobe=nlist)
        assert torch.equal(r_ivf, r_flat) and torch.equal(d_ivf, d_flat), (space, dtype, k)
    ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_masks_and_tombstones(env, space):
    torch, _, ivf = env
    n, d, nlist, B, nprobe, k = 3_000, 100, 24, 9, 5, 10
    c = Case(env, space, n, d, "f32", nlist, B, seed=77)
    try:
        assert c.install() == 0, native.last_error()
        mask = np.random.default_rng(9).random(n) < 0.10
        host = c.check(ivf, B, k, nprobe, mask=mask, what=(space, "host mask"))
        dev_words = torch.from_numpy(words_of(mask).view(np.int32)).to(c.ix.device)
        dev = keys_of(c.ix.ivf_search_keys_masked_dev(c.q[:B], dev_words, k, nprobe, ROW_BASE))
        assert np.array_equal(dev, host)
        dd, dr = c.ix.ivf_search_masked_dev_tensors(c.q[:B], dev_words, k, nprobe)
        want = c.expected(B, k, nprobe, mask)
        assert np.array_equal(dr.cpu().numpy(), want[2]) and np.array_equal(bits(dd.cpu().numpy()), bits(want[1]))
        # a mask that allows nothing
        nothing = np.zeros(n, dtype=bool)
        assert (keys_of(ivf.search_ivf_keys(c.ix, c.q[:B], k, nprobe, ROW_BASE, allow=nothing)) == 0).all()
        ed, er = ivf.search_ivf(c.ix, c.q[:B], k, nprobe, allow=nothing)
        assert bool((er == -1).all()) and bool(torch.isinf(ed).all()) and bool((ed > 0).all())
        # deletes leave the layout valid: the reference with those rows disallowed
        gone = np.unique(np.r_[c.twin, np.random.default_rng(10).choice(n, size=n // 8, replace=False)])
        c.ix.delete(gone)
        c.dead[gone] = True
        c.check(ivf, B, k, nprobe, what=(space, "deleted"))
        c.check(ivf, B, k, nprobe, mask=mask, what=(space, "deleted, masked"))
        gr = ivf.search_ivf(c.ix, c.q[:B], k, nprobe)[1].cpu().numpy()
        assert not np.isin(gr, gone).any()
        # an upsert makes the layout stale
        c.ix.upsert(np.array([7], dtype=np.int64), c.raw[:1], normalize=False)
        with pytest.raises(native.NativeLibraryError):
            ivf.search_ivf(c.ix, c.q[:B], k, nprobe)
        with pytest.raises(native.NativeLibraryError):
            ivf.search_ivf_keys(c.ix, c.q[:B], k, nprobe, allow=mask)
    finally:
        c.ix.close()


def test_two_ivf_shards_merge_to_the_whole_answer_under_l2(env):
    torch, Index, ivf = env
    from codd_query_engine_amd.sharded import ShardedSearcher

    n, d, k, cut, nlist = 6_000, 128, 10, 2_500, 8
    x, q = corpus(n, d, 32, 17, seed=8)

    def index_of(rows):
        ix = Index(d, dtype="f16", space="l2")
        ix.set_option("space_ivf", 1)
        ix.upsert(np.arange(rows.shape[0], dtype=np.int64), rows, normalize=False)
        return ix

    whole = index_of(x)
    qd = torch.from_numpy(q).to(whole.device)
    d_ref, r_ref = whole.search_tensors(qd, k)
    shards = []
    for lo, hi in ((0, cut), (cut, n)):
        s = index_of(x[lo:hi])
        ivf.build_ivf(s, nlist, iters=3)
        shards.append((lo, s))
    engines = [ivf.IvfShardEngine(s, nprobe=nlist) for _, s in shards]
    assert all(e.space == "l2" for e in engines)
    keys = torch.cat([e.search_keys(qd, k, lo) for e, (lo, _) in zip(engines, shards)], dim=1)
    _, d_got, r_got = whole.merge_keys(keys, k)
    assert torch.equal(r_got, r_ref) and torch.equal(d_got, d_ref)
    assert bool((d_got > 0).all()), "squared distances, not 1 - score"
    lo, s = shards[1]
    d1, r1 = ShardedSearcher(ivf.IvfShardEngine(s, nprobe=3), row_base=lo).search(qd, k)
    assert int(r1.min()) >= lo and bool((d1[:, 1:] >= d1[:, :-1]).all()) and bool((d1 >= 0).all())
    d_own, r_own = s.search_tensors(qd, k)
    hit = (r1 - lo) == r_own
    assert torch.equal(d1[hit], d_own[hit]), "a shard's hits carry the squared distances of its own flat search"
    for ix in (whole, shards[0][1], shards[1][1]):
        ix.close()


@pytest.mark.parametrize("space", sr.SPACES)
def test_build_quality(env, space):
    """k-means in the index's own space (means, exact assignment) on a clustered corpus: recall@10 against the index's own flat
    search never falls as nprobe grows, is 1.0 with every list probed and at least 0.90 with a quarter of them.  (A numpy
    restatement of the build rule on this corpus gives 1.00 for l2 and 0.98 .. 1.00 for ip at nprobe 16 over three seeds.)"""
    torch, Index, ivf = env
    n, d, nlist, k = 20_000, 64, 64, 10
    x, q = corpus(n, d, 128, 64, seed=12)
    ix = Index(d, dtype="f32", space=space)
    ix.set_option("space_ivf", 1)
    ix.upsert(np.arange(n, dtype=np.int64), x, normalize=False)
    stats = ivf.build_ivf(ix, nlist, iters=4)
    assert stats["rows"] == n and stats["nlist"] == nlist and 0 <= stats["min_list"] <= stats["max_list"] <= n
    assert abs(stats["mean_list"] * nlist - n) < 1e-6   # (the install refuses offsets that do not end at the row count)
    qd = torch.from_numpy(q).to(ix.device)
    d_flat, r_flat = ix.search_tensors(qd, k)
    recall = {}
    for nprobe in (1, 4, 16, 64):
        d_ivf, r_ivf = ivf.search_ivf(ix, qd, k, nprobe)
        recall[nprobe] = (r_ivf.unsqueeze(2) == r_flat.unsqueeze(1)).any(dim=2).float().mean().item()
        # a hit the flat search also returns carries the flat search's distance bits
        both = (r_ivf.unsqueeze(2) == r_flat.unsqueeze(1))
        i, a, b = both.nonzero(as_tuple=True)
        assert torch.equal(d_ivf[i, a], d_flat[i, b]), (space, nprobe)
    print("recall@10", space, recall)
    assert recall[1] <= recall[4] <= recall[16] <= recall[64], recall
    assert recall[64] == 1.0 and recall[16] >= 0.90, recall
    ix.close()


def test_a_build_puts_every_row_in_one_list(env):
    torch, Index, ivf = env
    n, d, nlist = 5_003, 64, 24
    x, _ = corpus(n, d, 48, 1, seed=4)
    ix = Index(d, dtype="f32", space="l2")
    ix.set_option("space_ivf", 1)
    ix.upsert(np.arange(n, dtype=np.int64), x, normalize=False)
    stats = ivf.build_ivf(ix, nlist, iters=2)
    assert stats["rows"] == n and abs(stats["mean_list"] * nlist - n) < 1e-6 and stats["min_list"] >= 0 and stats["max_list"] >= n / nlist
    # every row is in exactly one list: an exhaustive probe with k = 1 per row-as-query finds the row itself
    rows = torch.from_numpy(x[:64]).to(ix.device)
    r = ivf.search_ivf(ix, rows, 1, nlist)[1][:, 0].cpu().numpy()
    assert np.array_equal(r, np.arange(64))
    ix.close()


def test_opt_in(env, tmp_path):
    torch, Index, ivf = env
    from codd_query_engine_amd import KnnClient
    from codd_query_engine_amd.embedding import HashingEmbeddingFunction

    lib = native.load()
    # the option and the stat round-trip; 0 and 1 only
    c = Case(env, "l2", 3_000, 100, "f32", 24, 9, seed=77, option=0)
    try:
        assert c.ix.stat("space_ivf") == 0
        assert c.install() == -95 and "cosine" in native.last_error()       # off: nothing new is reachable
        assert lib.codd_knn_set_option(c.ix._h, b"space_ivf", 2) == -22
        c.ix.set_option("space_ivf", 1)
        assert c.ix.stat("space_ivf") == 1 and c.install() == 0
        keys = c.check(ivf, 9, 10, 5, what="on")
        c.ix.set_option("space_ivf", 0)                                      # off again: the searches refuse again
        assert c.ix.stat("space_ivf") == 0
        with pytest.raises(native.NativeLibraryError, match="cosine"):
            ivf.search_ivf_keys(c.ix, c.q, 10, 5, ROW_BASE)
        c.ix.set_option("space_ivf", 1)
        assert np.array_equal(keys_of(ivf.search_ivf_keys(c.ix, c.q, 10, 5, ROW_BASE)), keys)
        # a cosine index ignores the option: the same layout answers the same with it on and off
        cos = Index(100, dtype="f32")
        cos.upsert(np.arange(c.n, dtype=np.int64), c.raw)
        assert c.install(cos) == 0
        off = ivf.search_ivf_keys(cos, c.q, 10, 5)
        cos.set_option("space_ivf", 1)
        assert cos.stat("space_ivf") == 1 and c.install(cos) == 0
        assert torch.equal(ivf.search_ivf_keys(cos, c.q, 10, 5), off)
        cos.close()
    finally:
        c.ix.close()
    # the facade hands "codd:space_ivf" to the engine when it makes it, and again after a reload
    embed = HashingEmbeddingFunction(384)
    client = KnnClient(device="cuda:0", embedding_function=embed, path=str(tmp_path))
    col = client.get_or_create_collection("c", metadata={"hnsw:space": "l2", "codd:space_ivf": 1})
    col.upsert(ids=[f"id{i}" for i in range(40)], documents=[f"queue depth p99 #{i}" for i in range(40)])
    assert col._engine.space == "l2" and col._engine.stat("space_ivf") == 1 and col._engine.stat("space_filter") == 0
    ivf.build_ivf(col._engine, 4, iters=2)
    assert client.persist() == 1
    fresh = KnnClient(device="cuda:0", embedding_function=embed, path=str(tmp_path))
    again = fresh.get_or_create_collection("c")
    assert again._engine.stat("space_ivf") == 1
    col.upsert(ids=["late"], documents=["disk usage"])
    assert client.persist() == 1 and fresh.reload() == 1 and again._engine.stat("space_ivf") == 1 and again.count() == 41
    plain = client.get_or_create_collection("p", metadata={"hnsw:space": "l2"})
    plain.upsert(ids=["a", "b"], documents=["cpu", "memory"])
    assert plain._engine.stat("space_ivf") == 0
    if hasattr(embed, "close"):
        embed.close()
