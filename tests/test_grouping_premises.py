"""The conditions under which tests/test_gpu_grouping_capacity.py is where it claims to be, checked from tests/_grouping_reference.py
alone: every case has the stated items per thread, the IVF cases take the list-sharing scan and their pair histogram has the work-item
edges, the scoped batches name the scopes that matter, the two references equal the ones the suite already trusts, and the inputs
are not vacuous: in the numpy model of the lists, a base one too high for every thread's second list (what a per = 1 habit would
write) changes at least half of the expected answers.  No device, and no wrong kernel is ever run."""

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests import _grouping_reference as g
from tests import test_gpu_ivf_masked as im
from tests._scoped_oracle_engine import ScopedOracleEngine
from tests.test_gpu_deletes import expected_keys, stored


@pytest.fixture(scope="module")
def scoped():
    plan = g.ScopedPlan()
    rng = np.random.default_rng(3)
    raw = rng.standard_normal((plan.N, 64)).astype(np.float32)
    q = rng.standard_normal((g.MAX_BATCH, 64)).astype(np.float32)
    rows_st, qn = stored(raw, "f32"), o.normalize_rows(q)
    return plan, raw, rows_st, qn, q, g.space_key_table("cosine", rows_st, "f32", qn)


def test_the_thresholds_are_crossed_where_the_cases_say():
    plan = g.ScopedPlan()
    nlist = {s: plan.TOP[s] + 1 for s in plan.STAGES}
    assert [g.per_of(nlist[s]) for s in "abcd"] == [1, 2, 3, 5]
    assert nlist["a"] == g.THREADS and nlist["b"] == g.THREADS + 1
    # the scope table: its first allocation holds stage (a) exactly, and every later stage grows it between two searches
    assert 2 * nlist["a"] + 1 == g.OFFSETS_WORDS == g.offsets_words(nlist["a"]) and 2 * nlist["b"] + 1 == 2_051
    words = [g.offsets_words(nlist[s]) for s in "abcd"]
    assert words == [2_049, 4_097, 8_193, 16_385] and all(2 * nlist[s] + 1 <= w for s, w in zip("abcd", words))
    # bitmap blocks: 8,388,608 rows are the last count with one block per thread
    big = g.BlockPlan
    assert g.ROWS_PER_BLOCK == 32 * g.WORDS_PER_BLOCK and g.THREADS * g.ROWS_PER_BLOCK == big.STAGES[0]
    assert [g.blocks_of(n) for n in big.STAGES] == [1_024, 1_025, 1_026] and [g.per_of(g.blocks_of(n)) for n in big.STAGES] == [1, 2, 2]
    assert big.STAGES[1] % g.ROWS_PER_BLOCK == 1 and big.STAGES[2] % 32 != 0      # one word with one bit; a ragged last word
    # IVF lists per thread, and the batches
    assert [g.per_of(n) for n in (1_024, 1_025, 2_049, 3_000)] == [1, 2, 3, 3]
    assert g.smallest_shared_nprobe(256, 1_024) == 8 and [g.smallest_shared_nprobe(256, n) for n in (1_025, 2_049, 3_000)] == [9, 17, 24]
    assert plan.big_batch(1_024).shape == (g.MAX_BATCH,) and plan.big_batch(1_023).shape == (g.MAX_BATCH - 1,)


def test_the_scope_sizes_and_the_stage_writes(scoped):
    plan = scoped[0]
    sizes = np.bincount(plan.final, minlength=5_001)[1:]
    assert np.array_equal(sizes, plan.sizes[1:]) and plan.final.shape == (plan.N,)
    assert (sizes == 0).sum() >= 300 and all(plan.sizes[s] == 0 for s in (1, 1_023, 1_025))
    assert sorted(sizes[sizes > 100].tolist()) == [290, 300, 310] and (np.delete(sizes, np.array(plan.BIG) - 1) <= 5).all()
    run = np.flatnonzero(plan.final == 600)
    assert run[-1] - run[0] == run.size - 1 and run.size >= 4 * 64                 # whole waves of one scope
    assert plan.sizes[5_000] == 1 and plan.sizes[1_024] == 1 and 8_000 < plan.N <= 10_000
    # the writes of each stage lead to the labels the references use, the highest label ever set is the stage's, and what stage
    # (b) adds is one row
    lab, dead, top = np.zeros(plan.N, dtype=np.uint32), np.zeros(plan.N, dtype=bool), 0
    for stage in plan.STAGES:
        for verb, slots, labels in plan.writes(stage):
            if verb == "set":
                assert not dead[slots].any()
                lab[slots] = labels
                top = max(top, int(labels.max()))
            else:
                dead[slots] = True
        assert np.array_equal(lab, plan.labels(stage)) and np.array_equal(dead, plan.dead(stage)) and top == plan.TOP[stage], stage
    assert sum(s.size for _, s, _ in plan.writes("b")) == 1
    assert plan.deleted.size == 300 and np.isin(np.flatnonzero(plan.final == plan.EMPTIED), plan.deleted).all()
    assert not (plan.labels("f") == 5_000).any() and (plan.labels("e") == 5_000).sum() == 1     # the highest list ends empty, max_scope stays
    assert not (plan.labels("a") == 1_023).any()


@pytest.mark.parametrize("stage", list(g.ScopedPlan.STAGES))
def test_the_scoped_batches_name_the_scopes_that_matter(scoped, stage):
    plan, raw, rows_st, qn, _, key_of = scoped
    lab, dead, top = plan.labels(stage), plan.dead(stage), plan.TOP[stage]
    per = g.per_of(top + 1)
    live_size = np.bincount(lab[~dead], minlength=top + 2)
    batches = [plan.batch(stage, 256)] + ([plan.big_batch(1_024), plan.big_batch(1_023)] if stage == "d" else [])
    for scopes in batches:
        have = set(scopes.tolist())
        assert {0, 1_022, 1_023, 1_024, 1_025, plan.UNKNOWN, top, top + 1} <= have or scopes.shape[0] > 256
        assert scopes.dtype == np.uint32
        if scopes.shape[0] == 256:
            assert any(s != 0 and s <= top and live_size[s] == 0 for s in have), "an empty scope"
            assert any(s > top for s in have), "an unknown scope"
            if per >= 2:   # two non-empty scopes whose bases one thread writes: its first list and a later one
                same = [(a, b) for a in have for b in have if 0 < a < b <= top and a // per == b // per and live_size[a] and live_size[b]]
                assert same, (stage, per)
            if stage == "b":
                assert {2, 3} <= have and 2 // per == 3 // per == 1                  # scopes 2 t and 2 t + 1 of thread t = 1
        else:
            B = scopes.shape[0]
            assert 250 <= len(have) <= 310 and (scopes == 600).sum() == 300 == 75 * 4 and (scopes[1_020:] == 0).all()
            assert (scopes[:1_020] != 0).all() and (B == 1_024) == (scopes[1_020:].size == 4)
        # the inputs are not vacuous: the seeded defect changes at least half of the expected answers (nothing at per = 1)
        B = scopes.shape[0]
        good = g.scoped_keys(key_of[:B], lab, dead, top, scopes, 10)
        bad = g.scoped_keys(key_of[:B], lab, dead, top, scopes, 10, shift_second=True)
        changed = (good != bad).any(axis=1).sum()
        assert changed == 0 if per == 1 else changed >= B // 2, (stage, B, changed)
    small = plan.batch(stage, 5)
    assert small.tolist()[:4] == [7, 0, 1_023, 2] and small[4] == top


def test_scoped_keys_are_the_scoped_oracle_engine_s(scoped):
    plan, raw, rows_st, qn, q, key_of = scoped
    eng = ScopedOracleEngine(64, "f32")
    eng.upsert(np.arange(plan.N, dtype=np.int64), raw)
    lab = plan.labels("d")
    eng.set_scopes(np.arange(plan.N, dtype=np.int64), lab)
    assert np.array_equal(eng._rows, rows_st)
    none = np.zeros(plan.N, dtype=bool)
    for scopes, k in ((plan.batch("d", 256)[:48], 10), (plan.batch("d", 5), 100)):
        B = scopes.shape[0]
        want = eng.search_keys_scoped(q[:B], scopes, k, row_base=1_000)
        assert np.array_equal(g.scoped_subset_keys(rows_st, "f32", lab, none, 5_000, qn[:B], scopes, k, row_base=1_000), want)
        assert np.array_equal(g.scoped_keys(key_of[:B], lab, none, 5_000, scopes, k, row_base=1_000), want)
    # ... and with tombstones the selection from the table is still the oracle on the sub-matrix
    lab, dead, scopes = plan.labels("f"), plan.dead("f"), plan.batch("f", 256)[:64]
    want = g.scoped_subset_keys(rows_st, "f32", lab, dead, 5_000, qn[:64], scopes, 10, row_base=7)
    assert np.array_equal(g.scoped_keys(key_of[:64], lab, dead, 5_000, scopes, 10, row_base=7), want)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_subset_keys_equal_expected_keys_of_the_delete_tests(dtype):
    rng = np.random.default_rng(11)
    n, dim = 3_000, 64
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((9, dim)).astype(np.float32)
    rows_ref = stored(raw, dtype)
    see = (rng.random(n) < 0.20) & ~(rng.random(n) < 0.10)          # a 20 % mask, 10 % tombstones
    members = np.flatnonzero(see)
    for k, base in ((10, 0), (100, 1_000), (700, 5)):               # (700: more than the sub-matrix holds, padding)
        want = expected_keys(rows_ref, dtype, see, q, k, base)
        assert np.array_equal(g.subset_keys(rows_ref[members], members, dtype, o.normalize_rows(q), k, base), want), (dtype, k)
    assert (g.subset_keys(rows_ref[:0], members[:0], dtype, o.normalize_rows(q), 10) == 0).all()
    # remap_keys: the keys of the squeezed sub-matrix are the same keys with the rows renumbered
    new_slot = np.cumsum(see) - 1
    moved = g.remap_keys(expected_keys(rows_ref, dtype, see, q, 10, 0), new_slot)
    assert np.array_equal(moved, g.subset_keys(rows_ref[members], np.arange(members.size), dtype, o.normalize_rows(q), 10))


def test_ivf_reference_is_the_masked_ivf_test_s_reference_at_16_lists():
    rng = np.random.default_rng(12)
    n, dim, B = 2_000, 64, 40
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    c = im.Ctx()
    qn = o.normalize_rows(rng.standard_normal((B, dim)).astype(np.float32))
    c.assign = rng.integers(0, im.NLIST, n)
    c.key_of = im.key_table(stored(raw, "f32"), "f32", qn)
    _, c.probed = o.search(o.normalize_rows(rng.standard_normal((im.NLIST, dim)).astype(np.float32)), "f32", qn, im.NLIST)
    mask, dead = rng.random(n) < 0.3, rng.random(n) < 0.1
    for nprobe, base in ((8, 0), (3, 77), (im.NLIST, 1_000)):
        want = im.reference(c, B, nprobe, mask, dead, base)
        assert np.array_equal(g.ivf_reference(c.key_of, c.probed, c.assign, im.NLIST, B, nprobe, mask, dead, im.K, base), want)
        assert np.array_equal(g.ivf_reference(c.key_of, c.probed, c.assign, im.NLIST, B, nprobe, mask, dead, 3, base), want[:, :3])


@pytest.mark.parametrize("case", g.IVF_CASES, ids=[g.ivf_case_id(c) for c in g.IVF_CASES])
def test_the_ivf_cases_share_lists_and_their_pairs_cover_the_work_item_edges(case):
    space, dim, dtype, nlist, B, nprobe, k = case
    p = g.IvfPlan(space, dim, dtype, nlist, B)
    nprobe = nprobe or p.nprobe()
    assert g.shared_route_taken(B, nprobe, nlist, dtype, g.niter_of(dim, dtype)) and B * nprobe >= 2 * nlist
    if case[5] is None:
        assert not g.shared_route_taken(B, nprobe - 1, nlist, dtype, g.niter_of(dim, dtype)), "the smallest nprobe that shares"
    # the layout: skewed, about a third of the lists and the named ones empty
    sizes = np.diff(p.offsets)
    assert sizes.sum() == p.N and all(sizes[l] == 0 for l in p.forced_empty) and {0, nlist - 1} <= set(p.forced_empty)
    assert nlist <= 1_024 or {1_023, 1_024} <= set(p.forced_empty)
    assert (sizes == 0).mean() >= 0.30 and (sizes >= 200).sum() >= 2 and (sizes[p.private.ravel()] > 0).all()
    # the pairs per list: 0, 1, and every edge of the split into work items of IVF_NB = 4 pairs
    probed = p.probed(nprobe)
    assert probed.shape == (B, nprobe) and (np.sort(probed, axis=1)[:, 1:] != np.sort(probed, axis=1)[:, :-1]).all()
    hist = g.pairs_per_list(probed, nlist)
    assert hist.sum() == B * nprobe and {0, 1, 3, 4, 5, 8, 9} <= set(hist.tolist()) and hist.max() > 100, sorted(set(hist.tolist()))
    assert {g.IVF_NB - 1, g.IVF_NB, g.IVF_NB + 1, 2 * g.IVF_NB, 2 * g.IVF_NB + 1} <= set(hist.tolist())
    for grp, size in enumerate(p.GROUPS):       # a group's min(nprobe, PRIVATE) best private lists hold its pairs and nobody else's
        assert sorted(hist[p.private[grp]].tolist()) == [0] * (p.PRIVATE - min(nprobe, p.PRIVATE)) + [size] * min(nprobe, p.PRIVATE), (grp, size)
    assert hist[p.private[-1, 0]] == 129 and sizes[p.private[-1, 0]] >= 200      # 33 work items over one long list
    # not vacuous: the seeded defect changes the answer of at least half of the batch's DISTINCT queries.  (Counted over distinct
    # queries because a base that is off by one moves or loses at most one work item per list: of 129 copies that probe the same
    # lists only a handful can change, whatever the defect, and the copies are 158 of the 256.)
    good = p.expected(nprobe, k)
    bad = p.expected(nprobe, k, probed=g.shifted_probes(probed, nlist))
    changed = (good != bad).any(axis=1)
    distinct, hit = np.unique(p.qidx).size, np.unique(p.qidx[changed]).size
    print(g.ivf_case_id(case), "queries changed", int(changed.sum()), "of", B, "distinct", hit, "of", distinct)
    assert hit == 0 if g.per_of(nlist) == 1 else hit >= (distinct + 1) // 2, (hit, distinct)
    assert (good[:, 0] != 0).mean() > 0.9          # (a query whose probes are all empty lists has an empty answer: an edge, not the rule)


def test_the_block_plan_fixes_its_rows_before_any_exists():
    p = g.BlockPlan()
    n = p.n
    for b in p.EDGES:
        assert p.allowed[g.ROWS_PER_BLOCK * b - 3 : g.ROWS_PER_BLOCK * b + 4].all()
    assert p.allowed[0] and p.allowed[n - 1] and 3_000 <= p.allowed.sum() <= 3_100
    assert p.dead_final[5] and 2_150 <= p.dead_final.sum() <= 2_240 and 150 <= (p.dead_final & p.allowed).sum() <= 220
    word = g.ROWS_PER_BLOCK * 700 + 64
    assert word % 32 == 0 and p.dead_final[word : word + 32].all()
    assert len(set((np.flatnonzero(p.dead_final) // g.ROWS_PER_BLOCK).tolist())) >= 800          # spread over the blocks
    # every stage sees rows of its last block; stage 2's last block is one row, and it is visible
    for stage_n in p.STAGES:
        vis = p.visible(stage_n)
        assert vis.size > 2_800 and vis[-1] // g.ROWS_PER_BLOCK == g.blocks_of(stage_n) - 1, stage_n
    assert p.visible(p.STAGES[1])[-1] == p.STAGES[0]
    # compaction keeps more than 1,024 blocks; the windows lie inside the new count and their source rows are wanted
    assert p.live == n - p.dead_final.sum() and g.per_of(g.blocks_of(p.live)) == 2
    assert np.array_equal(p.new_slot[p.live_slots], np.arange(p.live))
    for first, cnt in p.windows:
        assert 0 <= first and first + cnt <= p.live
        p.at(p.live_slots[first : first + cnt])
    assert p.windows[-1] == (p.live - 8, 8) and p.live_slots[p.live - 1] == n - 1
    assert p.wanted.size < 3_200 and np.array_equal(p.at(p.visible(n)), np.flatnonzero(np.isin(p.wanted, p.visible(n))))
    # the chunks tile every stage's new rows
    lo = 0
    for stage_n in p.STAGES:
        parts = p.chunks(lo, stage_n)
        assert parts[0][0] == lo and sum(c for _, c, _ in parts) == stage_n - lo and all(c <= p.CHUNK for _, c, _ in parts)
        assert all(a // p.CHUNK == (a + c - 1) // p.CHUNK and s == a for a, c, s in parts)
        lo = stage_n
    assert len(p.chunks(0, p.STAGES[0])) == 8
