"""Thresholds, inputs and bit-exact references for tests/test_gpu_grouping_capacity.py (the device side) and
tests/test_grouping_premises.py (the conditions under which those tests are where they claim to be, without a device).

The list-driven routes group rows, pairs or bitmap blocks with prefix sums that ONE workgroup of 1,024 threads computes, thread t
taking per = ceil(items / 1,024) consecutive items (list_scan_kernels.h).  per = 1 is what every other test runs; the cases here
have per >= 2, the scope table past its first allocation, and batches up to the ABI's 1,024 queries.

Every reference is the CPU oracle on the sub-matrix the route may see (subset_keys), or a selection from a table that scores every
(query, row) pair once (ivf_reference).  No tolerance anywhere.  The seeded defect of the premises (a list base one too high for the
second item of each thread) lives in the numpy model of the lists below and nowhere else."""

from __future__ import annotations

import numpy as np

from oracle import knn_oracle as o
from tests import _k_boundary_cases as kb
from tests import _space_reference as sr
from tests.test_gpu_deletes import stored
from tests.test_gpu_ivf_masked import key_table

LOW = np.uint64(0xFFFFFFFF)
HIGH = np.uint64(0xFFFFFFFF00000000)

# ---- thresholds ------------------------------------------------------------------------------------------------------------------
THREADS = 1024             # scope_offsets_kernel, ivf_pair_offsets_kernel: one workgroup; scope_group_kernel: one thread per query
WORDS_PER_BLOCK = 256      # live_prefix_kernel, mask_prefix_kernel: bitmap words per workgroup ...
ROWS_PER_BLOCK = 8192      # ... = 32 x 256 rows per block total that scope_offsets_kernel turns into a block base
IVF_NB = 4                 # kIvfNB (geometry.h): the (query, list) pairs of one work item of ivf_scan_shared_kernel / ivf_shared_sq
MAX_BATCH = 1024           # CODD_KNN_MAX_BATCH
OFFSETS_WORDS = 2049       # the first allocation of the scope table (ensure_scope_lists): start[nlist + 1] and fill[nlist]


def per_of(items: int) -> int:
    """consecutive items per thread of a one-workgroup prefix sum: scopes (nlist = highest label + 1) in scope_offsets_kernel,
    IVF lists in ivf_pair_offsets_kernel, bitmap blocks in scope_offsets_kernel behind mask_prefix_kernel / live_prefix_kernel"""
    return (int(items) + THREADS - 1) // THREADS


def blocks_of(rows: int) -> int:
    """bitmap blocks of `rows` rows: what masked_search_body and codd_knn_compact pass to scope_offsets_kernel"""
    words = (int(rows) + 31) // 32
    return (words + WORDS_PER_BLOCK - 1) // WORDS_PER_BLOCK


def offsets_words(nlist: int) -> int:
    """the words the scope table holds once nlist lists were built (ensure_scope_lists: 2,049, then 2 cap - 1)"""
    cap = OFFSETS_WORDS
    while cap < 2 * nlist + 1:
        cap = 2 * cap - 1
    return cap


def niter_of(dim: int, dtype: str) -> int:
    """16-byte chunks per lane of a stored row (search_plan.h niter_of)"""
    return (o.pad_dim(dim) // (4 if dtype == "f32" else 8) + 63) // 64


def shared_route_taken(B: int, nprobe: int, nlist: int, dtype: str, niter: int) -> bool:
    """the condition of ivf_search_body under which the pairs are grouped by list (option ivf_share on)"""
    npairs = B * nprobe
    return npairs >= 1024 and npairs >= 2 * nlist and not (dtype != "f32" and niter == 4)


def smallest_shared_nprobe(B: int, nlist: int) -> int:
    return max(-(-2 * nlist // B), -(-1024 // B))


# ---- references ------------------------------------------------------------------------------------------------------------------
def subset_keys(rows_subset_stored, members, dtype, qn, k, row_base=0) -> np.ndarray:
    """u64 [B, k]: the oracle's keys of the sub-matrix `rows_subset_stored` (the stored rows of `members`, ascending global slots, and
    nothing else) with the row word rewritten to row_base + the global slot; 0 padded.  ScopedOracleEngine.search_keys_scoped's
    unpack / map / repack, for an index whose other rows the host never holds."""
    members = np.asarray(members, dtype=np.int64)
    keys = np.zeros((qn.shape[0], k), dtype=np.uint64)
    if members.size == 0:
        return keys
    assert rows_subset_stored.shape[0] == members.size and (np.diff(members) > 0).all()
    sub = o.search_keys(np.ascontiguousarray(rows_subset_stored), dtype, qn, k, 0)
    hit = sub != 0
    local = (LOW - (sub[hit] & LOW)).astype(np.int64)
    rows = (members[local] + row_base).astype(np.uint64)
    keys[hit] = (sub[hit] & HIGH) | (LOW - rows)
    return keys


def remap_keys(keys, new_slot_of, row_base=0) -> np.ndarray:
    """the same keys with every row r (global row = row_base + r) replaced by new_slot_of[r]"""
    keys = np.asarray(keys, dtype=np.uint64).copy()
    hit = keys != 0
    rows = (LOW - (keys[hit] & LOW)).astype(np.int64) - row_base
    keys[hit] = (keys[hit] & HIGH) | (LOW - (new_slot_of[rows] + row_base).astype(np.uint64))
    return keys


def scope_lists(labels, dead, nlist, shift_second=False):
    """numpy model of scope_count / scope_offsets / scope_scatter: (perm: the live slots grouped by label, start [nlist + 1]).
    shift_second: the seeded defect, the base of every thread's second list one too high (nothing at per = 1)"""
    live = np.flatnonzero(~dead)
    perm = live[np.argsort(labels[live], kind="stable")]
    start = np.zeros(nlist + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(labels[live], minlength=nlist))
    if shift_second and per_of(nlist) >= 2:
        start[:nlist][np.arange(nlist) % per_of(nlist) == 1] += 1
    return perm, start


def scope_members(perm, start, scope, max_scope):
    """ascending slots scope_scan_body hands to the scan for one query's scope"""
    if scope == 0:
        return np.sort(perm)
    if scope > max_scope:
        return np.zeros(0, dtype=np.int64)
    return np.sort(perm[start[scope] : max(start[scope], min(start[scope + 1], perm.size))])


def select_keys(key_of, member, k, row_base=0) -> np.ndarray:
    """u64 [B, k]: the k best of key_of[b] (row word = ~row) among the rows member[b] names; descending, 0 padded"""
    keys = np.where(member, key_of, np.uint64(0))
    top = np.zeros((keys.shape[0], k), dtype=np.uint64)
    kk = min(k, keys.shape[1])
    top[:, :kk] = np.sort(keys, axis=1)[:, ::-1][:, :kk]
    hit = top != 0
    top[hit] -= np.uint64(row_base)              # the row word is ~(row_base + row)
    return top


def scoped_subset_keys(rows_st, dtype, labels, dead, max_scope, qn, scopes, k, row_base=0) -> np.ndarray:
    """u64 [B, k]: per query the oracle's search over the sub-matrix of the live rows of its scope (one oracle call per scope)"""
    perm, start = scope_lists(labels, dead, max_scope + 1)
    scopes = np.asarray(scopes, dtype=np.int64)
    keys = np.zeros((scopes.shape[0], k), dtype=np.uint64)
    for s in np.unique(scopes):
        members = scope_members(perm, start, int(s), max_scope)
        sel = np.flatnonzero(scopes == s)
        keys[sel] = subset_keys(rows_st[members], members, dtype, np.ascontiguousarray(qn[sel]), k, row_base)
    return keys


def scoped_keys(key_of, labels, dead, max_scope, scopes, k, row_base=0, shift_second=False) -> np.ndarray:
    """u64 [B, k]: the same answers as a selection from key_of [B, n], which scores every (query, row) pair once in the index's
    space: the k best among the rows the model of the lists hands to query b's scope"""
    perm, start = scope_lists(labels, dead, max_scope + 1, shift_second)
    scopes = np.asarray(scopes, dtype=np.int64)
    member = np.zeros(key_of.shape, dtype=bool)
    for s in np.unique(scopes):
        row = np.zeros(key_of.shape[1], dtype=bool)
        row[scope_members(perm, start, int(s), max_scope)] = True
        member[scopes == s] = row
    return select_keys(key_of, member, k, row_base)


def ivf_reference(key_of, probed, assign, nlist, B, nprobe, mask, dead, k, row_base=0) -> np.ndarray:
    """u64 [B, k]: the k best of key_of[b] among the allowed live rows of the lists probed[b, :nprobe]; descending, 0 padded
    (reference() of tests/test_gpu_ivf_masked.py with nlist and k as parameters)"""
    in_lists = np.zeros((B, nlist + 1), dtype=bool)               # (a probe of -1 is no list)
    np.put_along_axis(in_lists, np.where(probed[:B, :nprobe] < 0, nlist, probed[:B, :nprobe]), True, axis=1)
    member = in_lists[:, assign] & (mask & ~dead)[None, :]
    return select_keys(key_of[:B], member, k, row_base)


def pairs_per_list(probed, nlist) -> np.ndarray:
    """the histogram of (query, list) pairs: what ivf_pair_count_kernel leaves in cnt[]"""
    return np.bincount(np.asarray(probed).ravel(), minlength=nlist)


def shifted_probes(probed, nlist, seed=0) -> np.ndarray:
    """numpy model of the seeded defect in ivf_pair_offsets_kernel: both bases of every thread's second list, pair_start and
    item_start, one too high.  The pairs stand grouped by list, inside a list in the order the scatter's atomics gave (here: seeded).
    The first position of such a list falls to the list before it, and the binary search over item_start no longer reaches the
    list's last work item, so the pairs of that item are never scanned.  -> the list each pair is scanned with, -1 = none"""
    probed = np.asarray(probed)
    flat = probed.ravel()
    order = np.lexsort((np.random.default_rng(seed).random(flat.size), flat))
    cnt = np.bincount(flat, minlength=nlist)
    start = np.zeros(nlist + 1, dtype=np.int64)
    start[1:] = np.cumsum(cnt)
    scanned = flat[order].copy()
    if per_of(nlist) >= 2:
        for l in np.flatnonzero((np.arange(nlist) % per_of(nlist) == 1) & (cnt > 0)):
            a, b = start[l], start[l + 1]
            scanned[a] = l - 1
            scanned[a + 1 + IVF_NB * ((cnt[l] + IVF_NB - 1) // IVF_NB - 1) : b] = -1
    out = np.empty_like(flat)
    out[order] = scanned
    return out.reshape(probed.shape)


def space_stored(space, raw, dtype):
    return stored(raw, dtype) if space == "cosine" else sr.stored(raw, dtype)


def space_queries(space, q):
    return o.normalize_rows(q) if space == "cosine" else sr.clean(q)


def space_key_table(space, rows_st, dtype, qprep) -> np.ndarray:
    """key_of[b, r]: the packed key of row r for query b (row word = ~r), every pair scored once"""
    if space != "l2":
        return key_table(rows_st, dtype, qprep)
    word = kb.score_words("l2", rows_st, dtype, qprep)
    return (word.astype(np.uint64) << np.uint64(32)) | (LOW - np.arange(rows_st.shape[0], dtype=np.uint64))[None, :]


def space_probes(space, cent, q, nprobe) -> np.ndarray:
    """[B, nprobe] lists by exact centroid score in the index's space, best first (the coarse index is an f32 index of that space)"""
    if space == "cosine":
        return o.search(o.normalize_rows(cent), "f32", o.normalize_rows(q), nprobe)[1]
    return sr.Reference(space, cent, "f32", q).topk(q.shape[0], nprobe)[2]


def unpack(space, keys, row_base=0):
    return kb.unpack(space, keys, row_base)


# ---- case 1 and 2: one index of 9,000 rows whose labels grow past 1,024, 2,048 and 4,096 scopes ----------------------------------------
class ScopedPlan:
    """Labels per stage, the deletes, and the batches.  Scope sizes: 0 .. 5 rows up to scope 2,048, 0 or 1 above; scopes 1, 1,023 and
    1,025 (and a few hundred others) empty; scopes 7, 600 and 1,500 about 300 rows, 600 in one run of slots (whole waves of one
    scope in scope_count_kernel)."""

    N = 9_000
    STAGES = "abcdef"
    BIG = (7, 600, 1_500)
    TOP = {"a": 1_023, "b": 1_024, "c": 2_048, "d": 5_000, "e": 5_000, "f": 5_000}     # max_scope per stage
    EMPTIED = 2_047                                                                    # stage (e) deletes every row of this scope
    UNKNOWN = 99_999

    def __init__(self, seed=41):
        rng = np.random.default_rng(seed)
        sizes = np.zeros(5_001, dtype=np.int64)
        sizes[1:1_024] = rng.integers(0, 6, 1_023)
        sizes[1_026:2_049] = rng.integers(0, 6, 1_023)
        sizes[2_049:5_000] = rng.random(2_951) < 0.5
        sizes[list(self.BIG)] = (300, 290, 310)
        sizes[[1, 1_023, 1_025]] = 0
        sizes[[2, 3, 1_022, 2_046, self.EMPTIED, 2_048, 2_049, 4_999]] = (2, 4, 3, 5, 4, 2, 1, 1)
        sizes[[1_024, 5_000]] = 1
        assert sizes.sum() < self.N - 500
        lab = np.zeros(self.N, dtype=np.uint32)
        lab[: sizes.sum()] = np.repeat(np.arange(5_001, dtype=np.uint32), sizes)
        lab = rng.permutation(lab)
        run = np.arange(4_000, 4_000 + sizes[600])                 # scope 600 in one run of slots
        out = np.setdiff1d(np.flatnonzero(lab == 600), run)
        into = run[lab[run] != 600]
        lab[out], lab[into] = lab[into], 600
        self.sizes, self.final = sizes, lab
        # stage (e): every row of one scope, 50 of a large one, and others at random: 300 in all
        gone = np.concatenate([np.flatnonzero(lab == self.EMPTIED), np.flatnonzero(lab == 7)[:50]])
        others = rng.permutation(np.setdiff1d(np.arange(self.N), np.concatenate([gone, np.flatnonzero(lab == 5_000)])))
        self.deleted = np.sort(np.concatenate([gone, others[: 300 - gone.size]]))
        self.highest_row = int(np.flatnonzero(lab == 5_000)[0])
        self.first_1023 = int(np.flatnonzero(lab == 1_022)[0])   # labelled 1,023 and back in stage (a): the highest scope is empty
        self.rng_seed = seed

    def labels(self, stage) -> np.ndarray:
        lab = np.where(self.final <= self.TOP[stage], self.final, 0).astype(np.uint32)
        if stage == "f":
            lab[self.highest_row] = 0
        return lab

    def dead(self, stage) -> np.ndarray:
        d = np.zeros(self.N, dtype=bool)
        if stage in "ef":
            d[self.deleted] = True
        return d

    def writes(self, stage):
        """the set_scopes / delete calls that take the index from the stage before to this one: [(verb, slots, labels)]"""
        if stage == "a":
            lab = self.labels("a")
            at = np.flatnonzero(lab)
            one = np.array([self.first_1023], dtype=np.int64)
            return [("set", at, lab[at]), ("set", one, np.array([1_023], dtype=np.uint32)), ("set", one, np.array([1_022], dtype=np.uint32))]
        if stage == "e":
            return [("delete", self.deleted, None)]
        if stage == "f":
            return [("set", np.array([self.highest_row], dtype=np.int64), np.zeros(1, dtype=np.uint32))]
        before = self.STAGES[self.STAGES.index(stage) - 1]
        at = np.flatnonzero(self.labels(stage) != self.labels(before))
        return [("set", at, self.labels(stage)[at])]

    def named_scopes(self, stage):
        """what every batch of 256 carries: scope 0, two scopes of one thread at per = 2 (2 t and 2 t + 1, t = 1), both sides of
        1,023 / 1,024, empty scopes, unknown ones, the highest of the stage and the one above it, the large ones"""
        top = self.TOP[stage]
        return [0, 2, 3, 1_022, 1_023, 1_024, 1_025, 1, self.UNKNOWN, top, top + 1, *self.BIG, 2_046, self.EMPTIED, 2_048, 2_049, 4_999, 5_000, 0]

    def batch(self, stage, B) -> np.ndarray:
        """the scopes of a batch of B queries at a stage"""
        if B == 5:
            return np.array([7, 0, 1_023, 2, self.TOP[stage]], dtype=np.uint32)
        named = self.named_scopes(stage)
        rng = np.random.default_rng(self.rng_seed + ord(stage) + B)
        rest = self.pool(stage, rng.random(B - len(named)) < 0.75)
        return rng.permutation(np.concatenate([named, rest]).astype(np.uint32))

    def pool(self, stage, edge=None) -> np.ndarray:
        """the labelled scopes of a stage; edge: only those that are a thread's first or second list (where one thread's running
        base starts and first moves).  Given a bool array: one scope per entry, from the edge pool where it is true."""
        lab = self.labels(stage)
        every = np.unique(lab[lab != 0])
        at_edge = every[every % per_of(self.TOP[stage] + 1) <= 1]
        if edge is None or edge is True:
            return every if edge is None else at_edge
        rng = np.random.default_rng(self.rng_seed + ord(stage))
        return np.where(edge, rng.choice(at_edge, size=len(edge)), rng.choice(every, size=len(edge)))

    def big_batch(self, B) -> np.ndarray:
        """case 2, at stage (d): about 300 distinct scopes, scope 600 carried by 300 queries (ranks 0 .. 299: 75 groups of 4), scope 0
        by the last queries of a batch of 1,024"""
        rng = np.random.default_rng(self.rng_seed + 1_024)
        pool = rng.choice(self.pool("d", True), size=298, replace=False)
        s = rng.choice(pool, size=MAX_BATCH).astype(np.uint32)
        s[rng.choice(1_020, size=300, replace=False)] = 600
        s[1_020:] = 0
        return s[:B]


# ---- case 3: more than 1,024 bitmap blocks ---------------------------------------------------------------------------------------------
class BlockPlan:
    """An index of up to 8,396,837 rows (dim 64, f16) made on the device in chunks: which rows a masked search may see, which are
    deleted, and which are read back, fixed before a row exists.  The host only ever holds the rows in `wanted`."""

    DIM, DTYPE = 64, "f16"
    STAGES = (8_388_608, 8_388_609, 8_396_837)        # 1,024 blocks; 1,025 (the last holds one word with one bit); 1,026, ragged
    CHUNK = 1 << 20
    EDGES = (1, 2, 511, 512, 1_023, 1_024, 1_025)

    def __init__(self, seed=53):
        rng = np.random.default_rng(seed)
        n = self.n = self.STAGES[-1]
        allowed = np.zeros(n, dtype=bool)
        for b in self.EDGES:
            allowed[ROWS_PER_BLOCK * b - 3 : ROWS_PER_BLOCK * b + 4] = True
        allowed[[0, n - 1]] = True
        allowed[rng.choice(n, size=3_000, replace=False)] = True
        dead = np.zeros(n, dtype=bool)
        dead[5] = True                                                            # compaction moves almost every row
        dead[rng.choice(np.flatnonzero(allowed)[1:-1], size=200, replace=False)] = True
        dead[rng.choice(n, size=2_000, replace=False)] = True
        dead[ROWS_PER_BLOCK * 700 + 64 : ROWS_PER_BLOCK * 700 + 96] = True        # one whole bitmap word
        dead[[ROWS_PER_BLOCK * 1_024, n - 1]] = False                             # stage 2's only new row and the tail stay visible
        self.allowed, self.dead_final = allowed, dead
        self.live_slots = np.flatnonzero(~dead)                                   # new slot -> source row
        self.new_slot = np.cumsum(~dead) - 1                                      # source row -> new slot (live rows)
        live = self.live = self.live_slots.size
        # read-back windows after compaction, in new slots: around the images of the block edges, the first rows, and the tail
        wins = [(0, 8)] + [(int(self.new_slot[ROWS_PER_BLOCK * b]) - 4, 8) for b in self.EDGES] + [(ROWS_PER_BLOCK * 1_024 - 4, 8), (live - 8, 8)]
        self.windows = wins
        want = allowed.copy()
        for first, cnt in wins:
            want[self.live_slots[first : first + cnt]] = True
        self.wanted = np.flatnonzero(want)

    def chunks(self, lo, hi):
        """[(first row, rows, seed)] of the device chunks that make rows [lo, hi): none crosses a multiple of CHUNK, the seed is the
        chunk's first row"""
        out = []
        while lo < hi:
            end = min(hi, (lo // self.CHUNK + 1) * self.CHUNK)
            out.append((lo, end - lo, lo))
            lo = end
        return out

    def visible(self, n) -> np.ndarray:
        """the slots a masked search over the first n rows may return"""
        return np.flatnonzero(self.allowed[:n] & ~self.dead_final[:n])

    def at(self, slots) -> np.ndarray:
        """positions in `wanted` of the given source rows"""
        pos = np.searchsorted(self.wanted, slots)
        assert np.array_equal(self.wanted[pos], slots)
        return pos


# ---- case 4: IVF layouts with more lists than threads ----------------------------------------------------------------------------------
class IvfPlan:
    """8,192 rows in hand-made lists.  Coordinates 0 .. 5 belong to six groups of identical queries (3, 4, 5, 8, 9 and 129 of them):
    group g's query is e_g, PRIVATE lists of group g have centroids near e_g, every other centroid and query is zero there.  So
    a group's queries probe its private lists first and nobody else does: those lists hold exactly 3, 4, 5, 8, 9 and 129 pairs,
    the edges of the kIvfNB = 4 split into work items."""

    N = 8_192
    GROUPS = (3, 4, 5, 8, 9, 129)
    PRIVATE = 24                      # private lists per group: the largest smallest-shared nprobe (nlist 3,000 at B = 256)

    def __init__(self, space, dim, dtype, nlist, B=256, seed=0):
        rng = np.random.default_rng(7_000 + nlist + dim + seed)
        self.space, self.dim, self.dtype, self.nlist, self.B = space, dim, dtype, nlist, B
        N, G, P = self.N, len(self.GROUPS), self.PRIVATE
        raw = rng.standard_normal((N, dim)).astype(np.float32)
        if space != "cosine":
            raw *= rng.uniform(0.5, 1.5, (N, 1)).astype(np.float32)
        self.raw = raw
        # centroids, unit length in every space: the probe order is the order by dot product
        cent = rng.standard_normal((nlist, dim))
        cent[:, :8] = 0.0
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        self.forced_empty = sorted({0, 1_023, 1_024, nlist - 1} & set(range(nlist)))
        free = np.setdiff1d(np.arange(nlist), self.forced_empty)
        self.private = rng.choice(free, size=(G, P), replace=False)
        for g in range(G):
            c = 0.3 * cent[self.private[g]]
            c[0] /= 6.0                                            # the group's first private list is its best probe
            c[:, g] = 1.0
            cent[self.private[g]] = c / np.linalg.norm(c, axis=1, keepdims=True)
        self.cent = cent.astype(np.float32)
        # rows -> lists: a third of the lists empty, heavy-tailed sizes, three lists of some hundred rows (one of them private to the
        # group of 129: 33 work items over one long list)
        w = np.where(rng.random(nlist) < 1 / 3, 0.0, rng.pareto(1.5, nlist) + 0.05)
        w[self.private.ravel()] = np.maximum(w[self.private.ravel()], 1.0)
        w[self.forced_empty] = 0.0
        heavy = [int(self.private[G - 1, 0]), int(free[len(free) // 3]), int(free[2 * len(free) // 3])]
        w[heavy] = 0.05 * w.sum()
        self.assign = rng.choice(nlist, size=N, p=w / w.sum())
        donors = np.flatnonzero(self.assign == heavy[1])
        for i, l in enumerate(np.setdiff1d(self.private.ravel(), self.assign)):      # no private list without rows: two from a long list
            self.assign[donors[2 * i : 2 * i + 2]] = l
        self.perm = np.argsort(self.assign, kind="stable").astype(np.int64)
        self.offsets = np.zeros(nlist + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum(np.bincount(self.assign, minlength=nlist))
        # queries: the groups' members scattered over the batch, the rest Gaussian outside the groups' coordinates
        nu = G + B - sum(self.GROUPS)
        uq = rng.standard_normal((nu, dim))
        uq[:, :8] = 0.0
        for g in range(G):
            uq[g] *= 0.05 / np.sqrt(dim)
            uq[g, g] = 1.0
        if space != "cosine":
            uq *= 1.3
        self.unique = uq.astype(np.float32)
        self.qidx = rng.permutation(np.concatenate([np.repeat(np.arange(G), self.GROUPS), np.arange(G, nu)]))
        self.queries = self.unique[self.qidx]
        self.mask = rng.random(N) < 0.30
        self.dead = np.zeros(N, dtype=bool)
        self.dead[rng.choice(N, size=N // 8, replace=False)] = True
        self._probed, self._key_of = {}, None

    def nprobe(self) -> int:
        return smallest_shared_nprobe(self.B, self.nlist)

    def probed(self, nprobe) -> np.ndarray:
        """[B, nprobe] lists of every query of the batch"""
        if nprobe not in self._probed:
            self._probed[nprobe] = space_probes(self.space, self.cent, self.unique, nprobe)[self.qidx]
        return self._probed[nprobe]

    def key_of(self) -> np.ndarray:
        if self._key_of is None:
            self._key_of = space_key_table(self.space, space_stored(self.space, self.raw, self.dtype), self.dtype, space_queries(self.space, self.unique))
        return self._key_of[self.qidx]

    def expected(self, nprobe, k, mask=None, dead=None, row_base=0, probed=None) -> np.ndarray:
        mask = np.ones(self.N, dtype=bool) if mask is None else mask
        dead = np.zeros(self.N, dtype=bool) if dead is None else dead
        probed = self.probed(nprobe) if probed is None else probed
        return ivf_reference(self.key_of(), probed, self.assign, self.nlist, self.B, nprobe, mask, dead, k, row_base)


# (space, dim, dtype, nlist, B, nprobe or None for the smallest shared one, k): every layout the device test installs
IVF_CASES = [("cosine", 64, "f32", nlist, 256, None, 10) for nlist in (1_024, 1_025, 2_049, 3_000)] + \
            [("cosine", 768, "bf16", nlist, 256, None, 10) for nlist in (1_024, 1_025, 2_049, 3_000)] + \
            [("l2", 64, "f32", 2_049, 256, None, 10), ("ip", 64, "f32", 2_049, 256, None, 10),
             ("cosine", 64, "f32", 2_049, 256, 128, 10), ("cosine", 64, "f32", 2_049, 256, None, 100), ("cosine", 64, "f32", 2_049, 1_024, 8, 10)]


def ivf_case_id(case) -> str:
    space, dim, dtype, nlist, B, nprobe, k = case
    return f"{space}-{dim}-{dtype}-L{nlist}-B{B}-p{nprobe or 'min'}-k{k}"
