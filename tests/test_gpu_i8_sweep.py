"""i8_sweep_kernel (csrc/filter_i8.h): the static six-step int8 tile program with the K order turned round on a
workgroup's tiles of odd ordinal, so that a tile stages two query slices instead of six.  int32 accumulation is associative: the
accumulators, the candidate lists and everything behind them must hold the same bits as under i8_tile_kernel<FILTER, 3, 16>.

Every case runs the same index and the same queries three times — "i8_sweep" 1, "i8_sweep" 0, "filter" 0 — and asserts that the
program named ran, that the candidate lists are equal as per-query sets of (row, score bits), that the survivor counts are equal and
that ids and distance bits are the exact scan's.  768-element f32 rows, k = 10; "debug_num_cus" (4 unless said otherwise) makes the
passes count that many compute units, so that a small corpus gives a workgroup several tiles.

A filter pass needs a sample of 2k = 20 tiles (search_plan.h: filter_applies), so the smallest corpus a pass runs on has 20 tiles.
The corpora of 256 and of 512 rows are therefore answered by the exact scan whatever "i8_sweep" says: those two cases assert that,
and the workgroups of exactly one tile (forward only: prologue and final drain) and of exactly two (one full pair) they stand for are
the 5,120-row corpus on 20 and on 10 compute units."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 10
D = 768


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(768_2_6)
    raw = rng.standard_normal((120_000, D), dtype=np.float32)
    q = rng.standard_normal((256, D), dtype=np.float32)
    for j in range(0, 256, 16):   # queries with real neighbours, in every tile range of the small corpora
        q[j] = raw[(j * 331) % 5_000] + 0.05 * rng.standard_normal(D, dtype=np.float32)
    return raw, q


def open_index(Index, raw, cus, **options):
    ix = Index(raw.shape[1], dtype="f32")
    ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw)
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)
    ix.set_option("shadow8", 1)
    ix.set_option("shadow8_cooldown", 0)
    ix.set_option("debug_num_cus", cus)
    for key, value in options.items():
        ix.set_option(key, value)
    return ix


def one_search(ix, q, sweep):
    ix.set_option("i8_sweep", sweep)
    before = {key: ix.stat(key) for key in ("filter_passes", "i8v2_passes", "sweep_passes", "filter_hits", "filter_survivors", "fallback_queries")}
    dist, rows = ix.search(q, K)
    delta = {key: ix.stat(key) - before[key] for key in before}
    return np.asarray(dist).copy(), np.asarray(rows).copy(), delta


def exact(ix, q):
    ix.set_option("filter", 0)
    dist, rows = ix.search(q, K)
    ix.set_option("filter", 1)
    return np.asarray(dist).copy(), np.asarray(rows).copy()


def assert_same_bits(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def compare(ix, q, expect_sweep=True, cascade_d=0):
    """the three searches of a case; returns the candidates per query"""
    B = q.shape[0]
    got = {}
    for sweep in (1, 0):
        dist, rows, delta = one_search(ix, q, sweep)
        lp = ix.last_pass()
        ran = (lp["family"], lp["ts"], lp["nbq"], lp["res"], lp["el"], lp["sweep"])
        want = ("TILE", 3, 8, 0, 1, int(bool(sweep and expect_sweep))) if expect_sweep else ran[:5] + (0,)
        assert ran == want, ("another program ran", ran, want)
        assert delta["filter_passes"] == 1 and delta["i8v2_passes"] == 1 and delta["sweep_passes"] == want[5], delta
        assert ix.stat("last_sweep") == want[5]
        assert lp["cascade_d"] == cascade_d, lp["cascade_d"]
        assert (lp["nq"], lp["k"]) == (B, K)
        assert int(lp["hit_counts"].astype(np.int64).max()) <= lp["hit_cap"], "a candidate list was cut: the sets below would be prefixes"
        got[sweep] = (dist, rows, delta, lp)
    (d1, r1, s1, lp1), (d0, r0, s0, lp0) = got[1], got[0]
    assert np.array_equal(lp1["thr"].view(np.uint32), lp0["thr"].view(np.uint32)) and np.array_equal(lp1["thr0"].view(np.uint32), lp0["thr0"].view(np.uint32))
    assert np.array_equal(lp1["hit_counts"], lp0["hit_counts"]), np.flatnonzero(lp1["hit_counts"] != lp0["hit_counts"])
    for qi in range(256):   # (row, score bits) are the two words of a key
        assert np.array_equal(np.sort(lp1["keys"][qi]), np.sort(lp0["keys"][qi])), qi
        assert qi < B or lp1["keys"][qi].size == 0, ("a padding query has candidates", qi)
    assert s1["filter_hits"] == s0["filter_hits"] and s1["filter_survivors"] == s0["filter_survivors"], (s1, s0)
    assert s1["fallback_queries"] == s0["fallback_queries"]
    ex = exact(ix, q)
    assert_same_bits((d1, r1), ex)
    assert_same_bits((d0, r0), ex)
    return lp1["hit_counts"].astype(np.int64)


@pytest.mark.parametrize("n", [256, 512])
def test_corpora_below_twenty_tiles_take_the_exact_scan_either_way(Index, data, n):
    raw, q = data
    ix = open_index(Index, raw[:n], 4)
    try:
        a = one_search(ix, q, 1)
        b = one_search(ix, q, 0)
        assert a[2]["filter_passes"] == 0 and b[2]["filter_passes"] == 0 and a[2]["sweep_passes"] == 0
        ex = exact(ix, q)
        assert_same_bits(a[:2], ex)
        assert_same_bits(b[:2], ex)
    finally:
        ix.close()


@pytest.mark.parametrize(
    "n,B,cus,options",
    [
        (5_120, 256, 20, {}),               # 20 tiles on 20 compute units: one tile per workgroup — forward only, prologue and final drain
        (5_120, 256, 10, {}),               # ... two per workgroup: one full pair
        (5_237, 256, 4, {}),                # 21 tiles: workgroups of 6, 5, 5 and 5 — both parities, the ragged last block on a backward tile
        (5_120, 256, 4, {}),                # 20 tiles, 5 each: the last tile forward ... (5,237: backward for workgroup 0)
        (5_120, 256, 3, {}),                # 7, 7, 6: the last tile forward for some workgroups and backward for others
        (5_237, 129, 4, {}),                # padding queries
        (5_237, 200, 4, {}),
        (5_237, 256, 4, {"per_block": 0}),  # the device-wide bound
    ],
)
def test_sweep_and_static_program_agree(Index, data, n, B, cus, options):
    raw, q = data
    ix = open_index(Index, raw[:n], cus, **options)
    try:
        counts = compare(ix, q[:B])
        assert counts[:B].sum() >= 10 * B, "too few candidates to tell two programs apart"
        print("n", n, "B", B, "cus", cus, options, "candidates", int(counts.sum()))
    finally:
        ix.close()


def test_non_positive_and_nan_thresholds(Index, data):
    """rows with positive components only: an all-negative query scores below zero against every row (its threshold is negative: the
    exact per-value test, no pre-test), a zero query has a NaN threshold"""
    raw, q = data
    q = q.copy()
    q[5] = 0.0
    q[7] = -np.abs(q[7])
    q[200] = -np.abs(q[200])
    ix = open_index(Index, np.abs(raw[:5_237]), 4)
    try:
        ix.set_option("i8_sweep", 1)
        compare(ix, q)
        lp = ix.last_pass()
        assert lp["thr"][7] < 0 and lp["thr"][200] < 0, (lp["thr"][7], lp["thr"][200])
    finally:
        ix.close()


def test_both_cascade_launches_sweep(Index, data):
    """120,000 rows on 32 compute units, the cascade forced on: launch A1 (every 17th tile) and launch B (the rest, under skip_d)"""
    raw, q = data
    ix = open_index(Index, raw, 32, sample_cascade=2)
    try:
        counts = compare(ix, q, cascade_d=16)
        assert ix.stat("cascade_passes") == 2
        assert counts.sum() >= 10 * 256
    finally:
        ix.close()


def test_candidate_and_survivor_counts_are_deterministic(Index, data):
    """a race in the hand-ordered schedule first shows as candidates that come and go between identical searches"""
    raw, q = data
    ix = open_index(Index, raw[:5_237], 4)
    try:
        runs = [one_search(ix, q, 1) for _ in range(10)]
        assert all(r[2]["sweep_passes"] == 1 for r in runs)
        assert len({(r[2]["filter_hits"], r[2]["filter_survivors"]) for r in runs}) == 1, [r[2] for r in runs]
        for r in runs[1:]:
            assert_same_bits(r[:2], runs[0][:2])
    finally:
        ix.close()


@pytest.mark.parametrize("d", [1536, 384])
def test_other_widths_keep_their_programs(Index, d):
    """12 K-steps (the pair program) and 3 (the resident one): the plan must not pick the sweep"""
    rng = np.random.default_rng(d)
    raw = rng.standard_normal((5_237, d), dtype=np.float32)
    q = rng.standard_normal((256, d), dtype=np.float32)
    ix = open_index(Index, raw, 4)
    try:
        compare(ix, q, expect_sweep=False)
        lp = ix.last_pass()
        assert lp["family"] == "TILE" and lp["ts"] != 3 and lp["sweep"] == 0
    finally:
        ix.close()
