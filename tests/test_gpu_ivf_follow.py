"""An IVF layout that follows writes on the GPU (option "ivf_follow", codd_knn_ivf_refresh).

The test installs layouts through codd_knn_ivf_install with its own centroids — `NLIST` of the rows — and its own assignment, the
top-1 of a centroid DeviceKnnIndex of the same space for the stored rows, so it knows every list's members; it tracks beside the
index which slots are pending, which are deleted and which list every slot of the layout sits in.  The references are the engine's
own flat searches: search_tensors for an exhaustive probe, search_masked_tensors under
(member of a probed list & ~pending) | pending for a partial one.  Everything is compared bit for bit, ids and distance bits."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NLIST = 16
FORMS = [(64, "f16", 6_001), (100, "f32", 6_001), (1536, "f32", 2_000)]    # counts that are no multiple of 32; 100: a ragged row; 1536: the wide form
SPACES = ["cosine", "l2", "ip"]
CASES = [(s, *f) for s in SPACES for f in FORMS]
NEVER = 1 << 32                                                            # "ivf_fold_rows": no write folds


class Env:
    pass


@pytest.fixture(scope="module", params=CASES, ids=[f"{s}-{d}-{t}" for s, d, t, _ in CASES])
def env(request):
    """per (space, row form): the corpus, the queries, the centroid index and the layout tables, made once and left unchanged"""
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import native
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    e = Env()
    e.space, e.dim, e.dtype, e.n = request.param
    e.torch, e.native, e.lib, e.Index = torch, native, native.load(), DeviceKnnIndex
    e.normalize = e.space == "cosine"
    rng = np.random.default_rng(2700 + e.dim + 7 * SPACES.index(e.space))
    e.raw = rng.standard_normal((e.n, e.dim)).astype(np.float32)
    if not e.normalize:
        e.raw *= rng.uniform(0.5, 1.5, size=(e.n, 1)).astype(np.float32)     # ip, l2: rows of different norms
    e.queries = rng.standard_normal((256, e.dim)).astype(np.float32)
    e.cent_rows = np.linspace(0, e.n - 1, NLIST).astype(np.int64)            # the centroids are NLIST of the rows
    e.cent = e.raw[e.cent_rows].copy()
    e.cidx = DeviceKnnIndex(e.dim, "f32", space=e.space)
    e.cidx.upsert_device(0, torch.from_numpy(e.cent).to(e.cidx.device), normalize=e.normalize)
    probe = fresh_index(e, follow=False)
    e.capacity0 = probe.stat("capacity_rows")
    e.assign = top1_lists(e, probe, np.arange(e.n))
    probe.close()
    e.perm = np.argsort(e.assign, kind="stable").astype(np.int64)
    e.offsets = np.zeros(NLIST + 1, dtype=np.int64)
    e.offsets[1:] = np.cumsum(np.bincount(e.assign, minlength=NLIST))
    yield e
    e.cidx.close()


def fresh_index(e, follow=True, fold_rows=NEVER):
    ix = e.Index(e.dim, e.dtype, space=e.space)
    ix.upsert(np.arange(e.n, dtype=np.int64), e.raw, normalize=e.normalize)
    if e.space != "cosine":
        ix.set_option("space_ivf", 1)
    if follow:
        ix.set_option("ivf_follow", 1)
        ix.set_option("ivf_fold_rows", fold_rows)
    return ix


def stored_f32(e, ix, first, n):
    out = e.torch.empty((n, e.dim), dtype=e.torch.float32, device=ix.device)
    e.native.check(e.lib.codd_knn_copy_rows_f32(ix._h, int(first), int(n), out.data_ptr(), ix._stream()), "codd_knn_copy_rows_f32")
    return out


def top1_lists(e, ix, slots):
    """the centroid index's top-1 for the STORED rows of `slots` (the fold's rule, and the rule the test's layout was made by)"""
    slots = np.asarray(slots, dtype=np.int64)
    out = np.empty(slots.shape[0], dtype=np.int64)
    if slots.size == 0:
        return out
    lo, hi = int(slots.min()), int(slots.max()) + 1
    lists = np.empty(hi - lo, dtype=np.int64)
    for a in range(lo, hi, 1024):
        c = min(1024, hi - a)
        lists[a - lo : a - lo + c] = e.cidx.search_tensors(stored_f32(e, ix, a, c), 1)[1][:, 0].cpu().numpy()
    return lists[slots - lo]


def install(e, ix):
    t = [e.torch.from_numpy(a).to(ix.device) for a in (e.cent, e.perm, e.offsets)]
    e.native.check(e.lib.codd_knn_ivf_install(ix._h, t[0].data_ptr(), NLIST, t[1].data_ptr(), t[2].data_ptr(), ix._stream()), "codd_knn_ivf_install")


class Tracked:
    """an index with an installed layout that follows writes, and what the test knows about it"""

    def __init__(self, e, fold_rows=NEVER):
        self.e, self.ix = e, fresh_index(e, fold_rows=fold_rows)
        install(e, self.ix)
        self.list_of = e.assign.copy()                # -1: not in the layout (appended since the last fold)
        self.pending = np.zeros(e.n, dtype=bool)
        self.dead = np.zeros(e.n, dtype=bool)
        self.refreshes = 0                            # folds seen so far ("ivf_refreshes")
        self.rng = np.random.default_rng(99)

    def close(self):
        self.ix.close()

    def count(self):
        return self.pending.shape[0]

    def vectors(self, n, near=None):
        """n new vectors; near: query numbers they lie close to, so that written rows turn up in answers"""
        v = self.rng.standard_normal((n, self.e.dim)).astype(np.float32)
        if near is not None:
            v = self.e.queries[np.resize(np.asarray(near), n)] + 0.3 * v
        return np.ascontiguousarray(v, dtype=np.float32)

    def _mark(self, slots, lo, hi):
        old = self.count()
        if hi > old:
            grow = hi - old
            self.pending = np.r_[self.pending, np.ones(grow, dtype=bool)]     # the gap and the appended slots: all pending
            self.dead = np.r_[self.dead, np.zeros(grow, dtype=bool)]
            self.list_of = np.r_[self.list_of, np.full(grow, -1, dtype=np.int64)]
        self.pending[slots] = True
        folds = self.ix.stat("ivf_refreshes")
        if folds != self.refreshes:                   # the write crossed "ivf_fold_rows" and folded before it returned
            assert folds == self.refreshes + 1 and self.ix.stat("ivf_pending_rows") == 0
            self.folded()

    def upsert(self, slots, vecs):
        slots = np.asarray(slots, dtype=np.int64)
        self.ix.upsert(slots, vecs, normalize=self.e.normalize)
        self._mark(slots, int(slots.min()), int(slots.max()) + 1)

    def upsert_device(self, first, vecs):
        self.ix.upsert_device(first, self.e.torch.from_numpy(vecs).to(self.ix.device), normalize=self.e.normalize)
        self._mark(np.arange(first, first + vecs.shape[0]), first, first + vecs.shape[0])

    def delete(self, slots):
        self.ix.delete(np.asarray(slots, dtype=np.int64))
        self.dead[slots] = True

    def folded(self):
        """the index has folded (ivf_refresh, or a write that crossed the threshold): the test's tables follow"""
        at = np.flatnonzero(self.pending)
        self.list_of[at] = top1_lists(self.e, self.ix, at)
        self.pending[:] = False
        self.refreshes = self.ix.stat("ivf_refreshes")
        assert (self.list_of >= 0).all() and self.ix.stat("ivf_rows") == self.count()

    def refresh(self):
        self.ix.ivf_refresh()
        assert self.ix.stat("ivf_refreshes") == self.refreshes + 1
        self.folded()

    def check_stats(self):
        assert self.ix.stat("ivf_pending_rows") == int(self.pending.sum())
        assert self.ix.count() == self.count()


def bits(t):
    return t.cpu().numpy().view(np.int32)


def assert_same(got, want, what):
    (gd, gr), (wd, wr) = got, want
    gr, wr = gr.cpu().numpy(), wr.cpu().numpy()
    assert np.array_equal(gr, wr), (what, "rows", np.flatnonzero((gr != wr).any(axis=1))[:4], gr[(gr != wr).any(axis=1)][:2], wr[(gr != wr).any(axis=1)][:2])
    assert np.array_equal(bits(gd), bits(wd)), (what, "distance bits")
    for row in gr:
        hit = row[row >= 0]
        assert np.unique(hit).shape[0] == hit.shape[0], (what, "a row id appears twice", row)


def check_exhaustive(t, what, ks=(1, 10, 100, 128), Bs=(1, 9)):
    """search_ivf(nprobe = nlist) is search_tensors, ids and distance bits"""
    from codd_query_engine_amd.ivf import search_ivf

    t.check_stats()
    for B in Bs:
        for k in ks:
            q = t.e.queries[:B]
            assert_same(search_ivf(t.ix, q, k, NLIST), t.ix.search_tensors(q, k), (what, B, k))


def probed_lists(e, q, nprobe):
    return e.cidx.search_tensors(q, nprobe)[1].cpu().numpy()


def partial_mask(t, lists):
    member = np.isin(t.list_of, lists)              # (-1, a slot outside the layout, is in no list)
    return (member & ~t.pending) | t.pending


def check_partial(t, what, nprobes=(1, 4), k=10, B=9, row_base=1000):
    """each query against the flat masked search over (members of ITS probed lists & ~pending) | pending; the keys form too"""
    from codd_query_engine_amd.ivf import search_ivf, search_ivf_keys

    t.check_stats()
    q = t.e.queries[:B]
    for nprobe in nprobes:
        lists = probed_lists(t.e, q, nprobe)
        dist, rows = search_ivf(t.ix, q, k, nprobe)
        keys = search_ivf_keys(t.ix, q, k, nprobe, row_base).cpu().numpy()
        for b in range(B):
            mask = partial_mask(t, lists[b])
            assert_same((dist[b : b + 1], rows[b : b + 1]), t.ix.search_masked_tensors(q[b : b + 1], mask, k), (what, nprobe, b))
            want = t.ix.search_keys_masked(q[b : b + 1], mask, k, row_base).cpu().numpy()
            assert np.array_equal(keys[b : b + 1], want), (what, "keys", nprobe, b)


@pytest.fixture()
def tracked(env):
    t = Tracked(env)
    yield t
    t.close()


def write_sequence(t):
    """the issue's write sequence, one step per yield"""
    e, n = t.e, t.e.n
    scattered = np.sort(t.rng.choice(n, size=37, replace=False))
    t.upsert(scattered, t.vectors(37, near=range(9)))
    yield "37 scattered slots through upsert_host"
    t.upsert_device(n // 3, t.vectors(200, near=range(9)))
    yield "a range through upsert_device"
    twice = int(scattered[5])
    t.upsert([twice], t.vectors(1))
    t.upsert([twice], t.vectors(1, near=[0]))
    yield "one slot twice with different vectors"
    t.upsert_device(t.count(), t.vectors(50, near=range(9)))
    yield "50 rows appended"
    t.upsert_device(t.count() + 10, t.vectors(20, near=range(9)))
    yield "an append that starts 10 slots above the count"
    assert t.ix.stat("capacity_rows") == e.capacity0
    more = e.capacity0 - t.count() + 7
    t.upsert_device(t.count(), t.vectors(more, near=range(9)))
    assert t.ix.stat("capacity_rows") > e.capacity0
    yield "an append that makes the row store grow"
    if t.pending.sum() < 40:                                     # (the append has folded: make some rows pending again)
        t.upsert(np.arange(200, 260), t.vectors(60, near=range(9)))
    pend, rest = np.flatnonzero(t.pending), np.flatnonzero(~t.pending)
    t.delete(np.r_[t.rng.choice(pend, size=40, replace=False), t.rng.choice(rest, size=40, replace=False)])
    yield "some pending and some other rows deleted"


def test_exhaustive_probe_equals_flat_after_every_write_and_after_the_fold(tracked):
    t = tracked
    check_exhaustive(t, "nothing pending", ks=(10,), Bs=(9,))
    for step in write_sequence(t):
        check_exhaustive(t, step)
    assert t.ix.stat("ivf_refreshes") == 0 and t.ix.stat("ivf_delta_searches") > 0
    t.refresh()
    assert t.ix.stat("ivf_pending_rows") == 0 and t.ix.stat("ivf_rows") == t.count()
    delta = t.ix.stat("ivf_delta_searches")
    check_exhaustive(t, "after the fold")
    assert t.ix.stat("ivf_delta_searches") == delta, "nothing pending: no delta scan"


def test_exhaustive_probe_equals_flat_when_writes_fold_at_the_default_threshold(env):
    """the same sequence with "ivf_fold_rows" at its default, one mean list: the large append folds on its own"""
    t = Tracked(env, fold_rows=0)
    try:
        assert t.ix.stat("ivf_fold_threshold") == -(-env.n // NLIST)
        for step in write_sequence(t):
            check_exhaustive(t, step, ks=(10, 128), Bs=(9,))
        assert t.refreshes >= 1
        check_partial(t, "after the sequence", nprobes=(4,))
    finally:
        t.close()


def test_partial_probe_with_rows_pending_and_after_the_fold(tracked):
    t = tracked
    for step in write_sequence(t):
        pass
    check_partial(t, "rows pending")
    before = t.ix.stat("ivf_refreshes")
    t.refresh()
    assert t.ix.stat("ivf_pending_rows") == 0 and t.ix.stat("ivf_refreshes") == before + 1
    check_partial(t, "after the fold")


def test_a_row_overwritten_near_another_centroid_is_found_there_after_the_fold(tracked):
    from codd_query_engine_amd.ivf import search_ivf

    t, e = tracked, tracked.e
    slot = int(np.flatnonzero((e.assign != 11) & ~np.isin(np.arange(e.n), e.cent_rows))[0])
    scale = 4.0 if e.space == "ip" else 1.0       # (ip: a long row, so that its product with itself is the largest in its list)
    vec = (scale * (e.cent[11] + 0.05 * t.rng.standard_normal(e.dim))).astype(np.float32)[None, :]
    t.upsert([slot], vec)
    assert search_ivf(t.ix, vec, 1, 1)[1].cpu().numpy()[0, 0] == slot, "pending: every query scans it"
    t.refresh()
    assert t.ix.stat("ivf_pending_rows") == 0
    assert t.list_of[slot] == probed_lists(e, vec, 1)[0, 0], "the query equal to the row probes the row's new list"
    if e.space != "ip":                               # (ip: the best centroid of a long row need not be the one it lies along)
        assert t.list_of[slot] == 11
    assert search_ivf(t.ix, vec, 1, 1)[1].cpu().numpy()[0, 0] == slot
    check_partial(t, "after the fold", nprobes=(1,))


def words_of(mask):
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((mask.shape[0] + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    return words.view("<u4").copy()


@pytest.mark.parametrize("form", ["host", "device"])
def test_masked_forms_with_rows_pending(tracked, form):
    from codd_query_engine_amd.ivf import search_ivf

    t, e = tracked, tracked.e
    slots = np.sort(t.rng.choice(e.n, size=37, replace=False))
    t.upsert(slots, t.vectors(37, near=range(9)))
    t.upsert_device(t.count(), t.vectors(20, near=range(9)))
    pend = np.flatnonzero(t.pending)
    t.delete(pend[::5])                                         # deleted pending rows
    q, k = e.queries[:9], 128

    def allow_of(mask):
        return e.torch.from_numpy(words_of(mask).view(np.int32)).to(t.ix.device) if form == "device" else mask

    # a mask that leaves half of the pending rows out
    mask = t.rng.random(t.count()) < 0.5
    mask[pend[1::2]] = False
    mask[pend[0::2]] = True
    got = search_ivf(t.ix, q, k, NLIST, allow=allow_of(mask))
    assert_same(got, t.ix.search_masked_tensors(q, mask, k), "half of the pending rows allowed")
    rows = got[1].cpu().numpy()
    assert not np.isin(rows, pend[1::2]).any(), "a pending row outside allow"
    assert not np.isin(rows, np.flatnonzero(t.dead)).any(), "a deleted pending row"
    assert np.isin(rows, pend[0::2]).any()
    # a mask that allows only pending rows: exactly the live ones, whatever is probed
    only = t.pending.copy()
    for nprobe in (1, NLIST):
        rows = search_ivf(t.ix, q, k, nprobe, allow=allow_of(only))[1].cpu().numpy()
        live = np.flatnonzero(t.pending & ~t.dead)
        assert live.shape[0] < k
        for b in range(q.shape[0]):
            assert sorted(rows[b][rows[b] >= 0]) == sorted(live), (nprobe, b)
    # ... and a partial probe under a mask: the flat masked search over the mask & the partial formula
    lists = probed_lists(e, q, 4)
    dist, rows = search_ivf(t.ix, q, 10, 4, allow=allow_of(mask))
    for b in range(q.shape[0]):
        assert_same((dist[b : b + 1], rows[b : b + 1]), t.ix.search_masked_tensors(q[b : b + 1], mask & partial_mask(t, lists[b]), 10), ("masked partial", b))


def test_shared_scan_with_rows_pending(tracked):
    from codd_query_engine_amd.ivf import search_ivf

    t, e = tracked, tracked.e
    t.upsert(np.sort(t.rng.choice(e.n, size=37, replace=False)), t.vectors(37, near=range(64)))
    t.upsert_device(t.count(), t.vectors(30, near=range(64)))
    q = e.queries[:256]                                          # 256 x 8 = 2,048 (query, list) pairs over 16 lists
    t.ix.set_option("ivf_share", 0)
    before = t.ix.stat("ivf_shared_searches")
    per_pair = search_ivf(t.ix, q, 10, 8)
    assert t.ix.stat("ivf_shared_searches") == before
    t.ix.set_option("ivf_share", 1)
    shared = search_ivf(t.ix, q, 10, 8)
    assert t.ix.stat("ivf_shared_searches") == before + 1
    assert_same(shared, per_pair, "ivf_share 1 against 0")
    assert_same(search_ivf(t.ix, q, 10, 8), per_pair, "a second call on the same scratch")
    # ... and both are the formula's answer
    lists = probed_lists(e, q[:3], 8)
    for b in range(3):
        assert_same((shared[0][b : b + 1], shared[1][b : b + 1]), t.ix.search_masked_tensors(q[b : b + 1], partial_mask(t, lists[b]), 10), ("shared", b))


def test_a_write_folds_when_it_crosses_ivf_fold_rows(env):
    t = Tracked(env, fold_rows=64)
    try:
        assert t.ix.stat("ivf_fold_rows") == 64 and t.ix.stat("ivf_fold_threshold") == 64
        t.upsert_device(100, t.vectors(64, near=range(9)))
        assert t.ix.stat("ivf_pending_rows") == 64 and t.ix.stat("ivf_refreshes") == 0
        check_exhaustive(t, "64 rows pending", ks=(10,))
        check_partial(t, "64 rows pending", nprobes=(4,))
        t.upsert([5], t.vectors(1, near=[0]))                     # the 65th pending row: this write folds
        assert t.ix.stat("ivf_pending_rows") == 0 and t.ix.stat("ivf_refreshes") == 1 and t.refreshes == 1
        delta = t.ix.stat("ivf_delta_searches")
        check_exhaustive(t, "after the automatic fold", ks=(10,))
        check_partial(t, "after the automatic fold", nprobes=(4,))
        assert t.ix.stat("ivf_delta_searches") == delta
        t.upsert_device(t.count(), t.vectors(65))                 # ... and an append that crosses it in one write
        assert t.ix.stat("ivf_pending_rows") == 0 and t.ix.stat("ivf_refreshes") == 2 and t.ix.stat("ivf_rows") == t.count()
        check_partial(t, "after the second fold", nprobes=(4,))
    finally:
        t.close()


def test_edge_cases(tracked):
    from codd_query_engine_amd.ivf import search_ivf

    t, e = tracked, tracked.e
    # a refresh with nothing pending is a no-op
    t.ix.ivf_refresh()
    assert t.ix.stat("ivf_refreshes") == 0 and t.ix.stat("ivf_delta_searches") == 0
    # fewer pending rows than k
    t.upsert([7, 4_000 % e.n, e.n - 1], t.vectors(3, near=[0, 1, 2]))
    check_exhaustive(t, "3 rows pending", ks=(10, 128))
    check_partial(t, "3 rows pending", nprobes=(1,))
    rows = search_ivf(t.ix, e.queries[:2], 10, 1, allow=t.pending.copy())[1].cpu().numpy()
    assert (np.sort(rows, axis=1)[:, -3:] == np.sort(np.flatnonzero(t.pending))).all() and (np.sort(rows, axis=1)[:, :-3] == -1).all()
    # all pending rows deleted
    t.delete(np.flatnonzero(t.pending))
    check_exhaustive(t, "every pending row deleted", ks=(10,))
    check_partial(t, "every pending row deleted", nprobes=(4,))
    t.refresh()
    check_exhaustive(t, "folded with deleted rows", ks=(10,))
    # follow off: EINVAL, nothing happens
    t.upsert([9], t.vectors(1))
    t.ix.set_option("ivf_follow", 0)
    with pytest.raises(e.native.NativeLibraryError, match="code -22"):
        t.ix.ivf_refresh()
    with pytest.raises(e.native.NativeLibraryError, match="rows changed"):
        search_ivf(t.ix, e.queries[:1], 10, 4)                    # rows left pending with the option off: a stale layout
    assert t.ix.stat("ivf_refreshes") == 1 and t.ix.stat("ivf_pending_rows") == 1
    t.ix.set_option("ivf_follow", 1)
    check_exhaustive(t, "follow on again", ks=(10,))
    # no layout: EINVAL
    bare = fresh_index(e)
    try:
        with pytest.raises(e.native.NativeLibraryError, match="code -22"):
            bare.ivf_refresh()
        assert bare.stat("ivf_refreshes") == 0
    finally:
        bare.close()
    for key, bad in (("ivf_follow", 2), ("ivf_follow", -1), ("ivf_fold_rows", -1)):
        with pytest.raises(e.native.NativeLibraryError, match="code -22"):
            t.ix.set_option(key, bad)


def test_follow_is_off_by_default_and_an_upsert_makes_the_layout_stale(env):
    from codd_query_engine_amd.ivf import search_ivf

    ix = fresh_index(env, follow=False)
    try:
        assert ix.stat("ivf_follow") == 0
        install(env, ix)
        search_ivf(ix, env.queries[:1], 10, 4)
        ix.upsert(np.array([3], dtype=np.int64), env.raw[:1], normalize=env.normalize)
        with pytest.raises(env.native.NativeLibraryError, match="rows changed since codd_knn_ivf_install"):
            search_ivf(ix, env.queries[:1], 10, 4)
        assert ix.stat("ivf_pending_rows") == 0 and ix.stat("ivf_delta_searches") == 0
    finally:
        ix.close()
