"""The list groupings past one item per thread: more than 1,024 scopes, more than 1,024 IVF lists, more than 1,024
bitmap blocks, and batches of 1,023 and 1,024 queries on the list-driven routes.  Every prefix sum behind these routes is one
workgroup of 1,024 threads that walks per = ceil(items / 1,024) items per thread; every other test stays at per = 1.

Inputs, thresholds and references: tests/_grouping_reference.py; that each case is where it claims to be: tests/
test_grouping_premises.py.  Every comparison is packed keys bit for bit against the CPU oracle on the rows the route may see; where
distances and rows are returned as well they must be those keys unpacked.  Every case asserts the stat that proves its route."""

import time

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _grouping_reference as g
from tests._scoped_oracle_engine import ScopedOracleEngine
from tests.test_gpu_deletes import stored
from tests.test_gpu_ivf_masked import words_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex, ivf


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_keys(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "queries", bad[:8], bad.size, got[bad[:1]], want[bad[:1]])


# ------------------------------------------------------------------------------------------------------------------------
# 1. scopes growing past the scope table's first allocation and past one scope per thread
# ------------------------------------------------------------------------------------------------------------------------
class ScopedRun:
    """One index of ScopedPlan.N rows, the checker engine that mirrors its writes (cosine), and key_of: every (query, row) pair
    scored once in the index's space.  A batch's queries are the first B of `queries`."""

    def __init__(self, Index, space, dim, dtype, unique):
        self.plan, self.space = g.ScopedPlan(), space
        rng = np.random.default_rng(100 + dim + len(space))
        n = self.plan.N
        raw = rng.standard_normal((n, dim)).astype(np.float32)
        if space != "cosine":
            raw *= rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
        uq = rng.standard_normal((unique, dim)).astype(np.float32)
        self.qidx = np.arange(g.MAX_BATCH) % unique
        self.queries = uq[self.qidx]
        self.ix = Index(dim, dtype=dtype, space=space)
        self.ix.upsert(np.arange(n, dtype=np.int64), raw, normalize=space == "cosine")
        rows_st = g.space_stored(space, raw, dtype)
        assert np.array_equal(self.ix.read_rows(0, n), rows_st)
        self.key_u = g.space_key_table(space, rows_st, dtype, g.space_queries(space, uq))
        self.eng = None
        if space == "cosine":
            self.eng = ScopedOracleEngine(dim, dtype)
            self.eng.upsert(np.arange(n, dtype=np.int64), raw)
        self.stage = None

    def apply(self, stage):
        for verb, slots, labels in self.plan.writes(stage):
            if verb == "set":
                self.ix.set_scopes(slots, labels)
                if self.eng:
                    self.eng.set_scopes(slots, labels)
            else:
                self.ix.delete(slots)
        self.stage, self.lab, self.dead, self.top = stage, self.plan.labels(stage), self.plan.dead(stage), self.plan.TOP[stage]
        assert self.ix.stat("scopes") == self.top and self.ix.live_count() == int((~self.dead).sum())
        if self.eng:
            assert np.array_equal(self.eng._labels(), self.lab)

    def expected(self, scopes, k, row_base=0):
        return g.scoped_keys(self.key_u[self.qidx[: len(scopes)]], self.lab, self.dead, self.top, scopes, k, row_base)

    def check(self, scopes, k, row_base=1_000):
        """keys under a row base, then distances and rows: both against the reference; two scoped searches counted"""
        B, ix = len(scopes), self.ix
        before = ix.stat("scoped_searches")
        want = self.expected(scopes, k, row_base)
        same_keys(u64(ix.search_keys_scoped(self.queries[:B], scopes, k, row_base)), want, (self.stage, B, k))
        if self.eng is not None and not self.dead.any() and B <= 5:     # the checker engine itself, where it has no tombstones to miss
            assert np.array_equal(self.eng.search_keys_scoped(self.queries[:B], scopes, k, row_base), want)
        dist, rows = ix.search_scoped(self.queries[:B], scopes, k)
        d_ref, r_ref = g.unpack(self.space, self.expected(scopes, k))
        assert np.array_equal(rows, r_ref) and np.array_equal(bits(dist), bits(d_ref)), (self.stage, B, k)
        assert ix.stat("scoped_searches") == before + 2
        return want


@pytest.mark.parametrize("space,dim,dtype,unique", [("cosine", 64, "f32", 256), ("cosine", 768, "bf16", 128), ("l2", 64, "f32", 32)],
                         ids=["cosine-64-f32", "cosine-768-bf16", "l2-64-f32"])
def test_scopes_grow_past_the_table_and_past_one_scope_per_thread(env, space, dim, dtype, unique):
    _, Index, _ = env
    run = ScopedRun(Index, space, dim, dtype, unique)
    plan = run.plan
    try:
        for stage in plan.STAGES:
            builds = run.ix.stat("scope_builds")
            run.apply(stage)
            assert g.per_of(run.top + 1) == {"a": 1, "b": 2, "c": 3}.get(stage, 5)
            scopes = plan.batch(stage, 256)
            want = run.check(scopes, 10)
            # unknown and empty scopes answer nothing, every other scope something; the named ones are among the former
            live_size = np.bincount(run.lab[~run.dead], minlength=run.top + 1)
            nothing = (scopes > run.top) | ((scopes != 0) & (live_size[np.minimum(scopes, run.top)] == 0))
            assert nothing[np.isin(scopes, [plan.UNKNOWN, run.top + 1, 1, 1_023, 1_025])].all() and nothing.sum() < 64
            assert nothing[scopes == plan.EMPTIED].all() == (stage in "abef") and nothing[scopes == 5_000].all() == (stage != "e" and stage != "d")
            assert (want[nothing] == 0).all() and (want[~nothing][:, 0] != 0).all()
            run.check(plan.batch(stage, 5), 100)
            print(f"stage ({stage}): highest scope {run.ix.stat('scopes')}, per {g.per_of(run.top + 1)}, table words {g.offsets_words(run.top + 1)}, "
                  f"builds {run.ix.stat('scope_builds')}, scoped searches {run.ix.stat('scoped_searches')}, empty answers {int(nothing.sum())} of 256")
            assert run.ix.stat("scope_builds") == builds + 1, stage     # built once per stage: between two searches, never twice
    finally:
        run.ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. batches of 1,023 and 1,024 on the scoped and the masked list route
# ------------------------------------------------------------------------------------------------------------------------
def test_batches_of_1023_and_1024_on_the_list_driven_routes(env):
    torch, Index, _ = env
    run = ScopedRun(Index, "cosine", 64, "f32", g.MAX_BATCH)
    plan, ix = run.plan, run.ix
    try:
        for stage in "abcd":
            run.apply(stage)
        for B in (g.MAX_BATCH, g.MAX_BATCH - 1):
            scopes = plan.big_batch(B)
            want = run.check(scopes, 10)
            carried = np.flatnonzero(scopes == 600)
            assert carried.size == 300 and (want[carried][:, 9] != 0).all()          # ranks 0 .. 299 of one scope: 75 groups of 4
            everyone = u64(ix.search_keys(run.queries[1_020:1_021], 10, row_base=1_000))
            assert np.array_equal(want[1_020], everyone[0])                          # scope 0, carried by the last queries: the flat search
        assert ix.stat("scope_builds") == 1
        # the masked list route, with the tombstones of stage (e)
        run.apply("e")
        ix.set_option("mask_route", 1)
        n = plan.N
        mask = np.random.default_rng(5).random(n) < 0.03
        words = words_of(mask)
        dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
        member = np.broadcast_to(mask & ~run.dead, (g.MAX_BATCH, n))
        for B in (g.MAX_BATCH, g.MAX_BATCH - 1):
            for k in (10, 65):
                before = ix.stat("mask_list_searches")
                want = g.select_keys(run.key_u[run.qidx[:B]], member[:B], k, 1_000)
                same_keys(u64(ix.search_keys_masked(run.queries[:B], words, k, 1_000)), want, ("masked host", B, k))
                same_keys(u64(ix.search_keys_masked_dev(run.queries[:B], dev_words, k, 1_000)), want, ("masked dev", B, k))
                d_ref, r_ref = o.unpack_keys(g.select_keys(run.key_u[run.qidx[:B]], member[:B], k))
                for dist, rows in (ix.search_masked(run.queries[:B], mask, k), ix.search_masked_dev(run.queries[:B], dev_words, k)):
                    assert np.array_equal(rows, r_ref) and np.array_equal(bits(dist), bits(d_ref)), (B, k)
                assert ix.stat("mask_list_searches") == before + 4 and ix.stat("mask_dense_searches") == 0
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. more than 1,024 bitmap blocks: the masked list route and compaction
# ------------------------------------------------------------------------------------------------------------------------
def test_more_than_1024_bitmap_blocks_on_the_masked_list_route_and_in_compaction(env):
    """8,388,608 rows of dim 64 in f16 (1 GiB) are the threshold itself: 1,024 blocks of 8,192 rows.  The rows are made on the device
    in chunks and the host keeps the raw values of the rows it will ask about, nothing else."""
    torch, Index, _ = env
    p = g.BlockPlan()
    dim, dtype, k, base = p.DIM, p.DTYPE, 10, 1_000
    rng = np.random.default_rng(8)
    q = rng.standard_normal((64, dim)).astype(np.float32)
    # queries 0 .. 6 become copies of rows at the edges of the last blocks once those rows exist: their answers begin there
    planted = [p.n - 1, g.ROWS_PER_BLOCK * 1_025, g.ROWS_PER_BLOCK * 1_024 + 3, g.ROWS_PER_BLOCK * 1_024, g.ROWS_PER_BLOCK * 1_024 - 1,
               g.ROWS_PER_BLOCK * 1_023 + 2, 0]
    ix = Index(dim, dtype=dtype)
    t0 = time.perf_counter()
    try:
        ix.reserve(p.n)
        ix.set_option("mask_route", 1)
        raw_w = np.zeros((p.wanted.size, dim), dtype=np.float32)
        lo, before_compaction = 0, {}
        for n in p.STAGES:
            for first, cnt, seed in p.chunks(lo, n):
                gen = torch.Generator(device=ix.device)
                gen.manual_seed(seed)
                t = torch.randn((cnt, dim), generator=gen, device=ix.device, dtype=torch.float32)
                ix.upsert_device(first, t)
                a, b = np.searchsorted(p.wanted, [first, first + cnt])
                if b > a:
                    raw_w[a:b] = t[torch.from_numpy(p.wanted[a:b] - first).to(ix.device)].cpu().numpy()
                del t
            ix.delete(np.flatnonzero(p.dead_final[lo:n]) + lo)
            lo = n
            assert ix.count() == n and ix.live_count() == n - int(p.dead_final[:n].sum())
            assert g.blocks_of(n) == {p.STAGES[0]: 1_024, p.STAGES[1]: 1_025}.get(n, 1_026)
            st_w = stored(raw_w, dtype)                                   # (rows not made yet are zeros, and not asked about)
            if n == p.STAGES[0]:   # the stored form of rows made on the device is the oracle's: a block edge read back
                edge = np.arange(g.ROWS_PER_BLOCK * 512 - 3, g.ROWS_PER_BLOCK * 512 + 4)
                assert np.array_equal(ix.read_rows(int(edge[0]), edge.size), st_w[p.at(edge)])
            vis = p.visible(n)
            twins = [r for r in planted if r in vis] + [int(vis[-1])]
            twins = twins[-1:] + twins[:-1]                              # (the last visible row first: B = 1 asks for it)
            q[: len(twins)] = raw_w[p.at(np.array(twins))][:, :dim]
            qn = o.normalize_rows(q)
            words = words_of(p.allowed[:n])
            dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
            for B in (1, 9, 64):
                calls = ix.stat("mask_list_searches")
                want = g.subset_keys(st_w[p.at(vis)], vis, dtype, qn[:B], k, base)
                assert g.unpack("cosine", want, base)[1][: len(twins), 0].tolist() == twins[:B], "each planted query's best row is its twin"
                same_keys(u64(ix.search_keys_masked(q[:B], words, k, base)), want, ("host words", n, B))
                same_keys(u64(ix.search_keys_masked_dev(q[:B], dev_words, k, base)), want, ("device words", n, B))
                assert ix.stat("mask_list_searches") == calls + 2
                before_compaction[B] = want
            print(f"{n:,} rows: {g.blocks_of(n):,} blocks, per {g.per_of(g.blocks_of(n))}, {vis.size:,} visible, live {ix.live_count():,}, "
                  f"list searches {ix.stat('mask_list_searches')}, {time.perf_counter() - t0:.2f} s so far")
        # compaction: new slot = rank among the live rows
        t1 = time.perf_counter()
        assert ix.compact() == p.live and ix.count() == p.live == ix.live_count() and ix.stat("compactions") == 1 and ix.stat("dead_rows") == 0
        print(f"compacted to {ix.count():,} rows ({g.blocks_of(ix.count()):,} blocks) in {time.perf_counter() - t1:.2f} s")
        for first, cnt in p.windows:
            src = p.live_slots[first : first + cnt]
            assert np.array_equal(ix.read_rows(first, cnt), st_w[p.at(src)]), ("window at new slot", first, "source rows", src[:2])
        with pytest.raises(native.NativeLibraryError):
            ix.read_rows(p.live - 1, 2)
        vis = p.visible(p.n)
        moved = np.zeros(p.live, dtype=bool)
        moved[p.new_slot[vis]] = True
        words = words_of(moved)
        dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
        for B in (1, 9, 64):
            calls = ix.stat("mask_list_searches")
            want = g.subset_keys(st_w[p.at(vis)], p.new_slot[vis], dtype, qn[:B], k, base)
            assert np.array_equal(want, g.remap_keys(before_compaction[B], p.new_slot, base))      # the same keys, the rows renumbered
            same_keys(u64(ix.search_keys_masked(q[:B], words, k, base)), want, ("compacted, host words", B))
            same_keys(u64(ix.search_keys_masked_dev(q[:B], dev_words, k, base)), want, ("compacted, device words", B))
            assert ix.stat("mask_list_searches") == calls + 2
        assert ix.stat("mask_dense_searches") == 0 and ix.stat("shadow8_builds") == 0
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. IVF with more lists than threads
# ------------------------------------------------------------------------------------------------------------------------
MASKED_CASE = ("cosine", 64, "f32", 2_049, 256, None, 10)


@pytest.mark.parametrize("case", g.IVF_CASES, ids=[g.ivf_case_id(c) for c in g.IVF_CASES])
def test_ivf_with_more_lists_than_threads(env, case):
    torch, Index, ivf = env
    space, dim, dtype, nlist, B, nprobe, k = case
    p = g.IvfPlan(space, dim, dtype, nlist, B)
    nprobe = nprobe or p.nprobe()
    assert g.shared_route_taken(B, nprobe, nlist, dtype, g.niter_of(dim, dtype))
    ix = Index(dim, dtype=dtype, space=space)
    try:
        if space != "cosine":
            ix.set_option("space_ivf", 1)
        ix.upsert(np.arange(p.N, dtype=np.int64), p.raw, normalize=space == "cosine")
        t = [torch.from_numpy(a).to(ix.device) for a in (p.cent, p.perm, p.offsets)]
        rc = native.load().codd_knn_ivf_install(ix._h, t[0].data_ptr(), nlist, t[1].data_ptr(), t[2].data_ptr(), ix._stream())
        assert rc == 0, native.last_error()

        def both_scans(want, search, calls, what):
            """the per-pair scan, then the shared scan twice: all three the reference's keys; one shared search counted per call"""
            ix.set_option("ivf_share", 0)
            shared = ix.stat("ivf_shared_searches")
            per_pair = search()
            assert ix.stat("ivf_shared_searches") == shared
            ix.set_option("ivf_share", 1)
            first = search()
            assert ix.stat("ivf_shared_searches") == shared + calls
            again = search()                                     # the counters were cleared on the way: the grouping scratch is reused
            assert ix.stat("ivf_shared_searches") == shared + 2 * calls
            same_keys(first, want, (what, "shared"))
            same_keys(per_pair, first, (what, "per pair"))
            same_keys(again, first, (what, "second shared call"))

        want = p.expected(nprobe, k, row_base=77)
        both_scans(want, lambda: u64(ivf.search_ivf_keys(ix, p.queries, k, nprobe, 77)), 1, "plain")
        dist, rows = ivf.search_ivf(ix, p.queries, k, nprobe)
        d_ref, r_ref = g.unpack(space, p.expected(nprobe, k))
        assert np.array_equal(rows.cpu().numpy(), r_ref) and np.array_equal(bits(dist.cpu().numpy()), bits(d_ref))
        hist = g.pairs_per_list(p.probed(nprobe), nlist)
        print(f"{nlist:,} lists, per {g.per_of(nlist)}, {B * nprobe:,} pairs, {int((hist > 0).sum()):,} lists probed, most pairs on one list {int(hist.max())}, "
              f"shared searches {ix.stat('ivf_shared_searches')}")
        if case == MASKED_CASE:   # a 30 % mask over tombstones set after the install, host words and device words
            ix.delete(np.flatnonzero(p.dead))
            words = words_of(p.mask)
            dev_words = torch.from_numpy(words.view(np.int32)).to(ix.device)
            want = p.expected(nprobe, k, mask=p.mask, dead=p.dead, row_base=77)

            def masked():
                host = u64(ix.ivf_search_keys_masked(p.queries, words, k, nprobe, 77))
                dev = u64(ix.ivf_search_keys_masked_dev(p.queries, dev_words, k, nprobe, 77))
                same_keys(dev, host, "device words against host words")
                return host

            both_scans(want, masked, 2, "masked")
            both_scans(p.expected(nprobe, k, dead=p.dead, row_base=77), lambda: u64(ivf.search_ivf_keys(ix, p.queries, k, nprobe, 77)), 1, "tombstones")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the façade past 1,024 namespaces
# ------------------------------------------------------------------------------------------------------------------------
def test_the_facade_past_1024_namespaces():
    from codd_query_engine_amd import KnnClient

    rng = np.random.default_rng(9)
    spaces, dim = 1_100, 48
    n = 3 * spaces
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    names = [f"team-{i:04d}:svc" for i in range(spaces)]
    md = [{"namespace": names[i % spaces], "k": i} for i in range(n)]        # first seen first: namespace i is scope i + 1

    def filled(client):
        col = client.get_or_create_collection("many")
        col.upsert(ids=[f"id{i}" for i in range(n)], embeddings=vecs, metadatas=md)
        return col

    device, checker = filled(KnnClient(device="cuda:0")), filled(KnnClient(engine_factory=lambda d: ScopedOracleEngine(d)))
    q = rng.standard_normal((4, dim)).astype(np.float32)
    asked = [names[0], names[1_023], names[1_024], names[-1]]                  # scopes 1, 1,024, 1,025 and 1,100
    for name in asked:
        got = device.query(query_embeddings=q, n_results=5, where={"namespace": name})
        want = checker.query(query_embeddings=q, n_results=5, where={"namespace": name})
        assert got["ids"] == want["ids"] and got["distances"] == want["distances"], name
        assert all(len(ids) == 3 for ids in got["ids"]) and all(m["namespace"] == name for m in got["metadatas"][0])
    per_query = [{"namespace": name} for name in asked]
    got, want = device.query(query_embeddings=q, n_results=5, where=per_query), checker.query(query_embeddings=q, n_results=5, where=per_query)
    assert got["ids"] == want["ids"] and got["distances"] == want["distances"]
    assert [m[0]["namespace"] for m in got["metadatas"]] == asked
    engine = device._engine
    print(f"{engine.count():,} rows, highest scope {engine.stat('scopes')}, scoped searches {engine.stat('scoped_searches')}, builds {engine.stat('scope_builds')}")
    assert engine.stat("scopes") == spaces and g.per_of(spaces + 1) == 2
    assert engine.stat("scoped_searches") == 5 and engine.stat("scope_builds") == 1
