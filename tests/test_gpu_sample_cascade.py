"""The sample cascade (csrc/search_plan.h: cascade_plan): a pass of the static int8 tile program fixes its thresholds
in two steps — a one-round sample A0, then the filter program itself over tiles 0, d + 1, 2 (d + 1), ... (A1), whose candidates
stay in the hit lists — and the main launch B skips A1's tiles.  Only time may change: ids and distances must equal, bit for bit,
the exact scan's ("filter" = 0) and the plain pass's ("sample_cascade" = 0).  B never sees A1's tiles, so a candidate A1 loses is
lost for good: the planted rows, the tombstones and the empty sampled tiles below are there for that.

768-wide f32 rows and 256 queries unless a case says otherwise; "sample_cascade" = 2 (wherever the cascade applies).  The cases are laid
out for d = 32 ("cascade_d"); test_default_d runs the shipped d = 16.  k = 64 goes through the cascade on the 600k-row corpus only: the
first sample needs 2k = 128 tiles, which the two smaller corpora of the issue do not have, so their k = 64 cases compare the plain pass
(or, at 100 tiles, the exact scan it falls back to) with the exact scan."""

import numpy as np
import pytest

from tests import _filter_stage_reference as fs

pytestmark = pytest.mark.gpu

DIM, D = 768, 32
TILE_ROWS = 256


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def Index(torch_):
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def new_index(Index, torch_, n, seed, ranges=None):
    """n rows of seeded Gaussian noise, generated and stored on the device; ranges: only these [lo, hi) are written"""
    g = torch_.Generator(device="cuda").manual_seed(seed)
    ix = Index(DIM, dtype="f32")
    ix.reserve(n)
    for lo, hi in ranges or [(0, n)]:
        for a in range(lo, hi, 1 << 18):
            b = min(hi, a + (1 << 18))
            ix.upsert_device(a, torch_.randn((b - a, DIM), generator=g, device="cuda", dtype=torch_.float32))
    torch_.cuda.synchronize()
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)
    ix.set_option("cascade_d", D)
    assert ix.count() == n
    return ix


def queries(n_queries, seed):
    return np.random.default_rng(seed).standard_normal((n_queries, DIM)).astype(np.float32)


def three_ways(ix, q, k, cascade=True, keys_per_query=1, d=D):
    """the search with the cascade forced, without it, and by the exact scan, all three equal bit for bit: (dist, rows, counters
    moved, last_pass) of the first"""
    out = {}
    for name, options in (("cascade", {"filter": 1, "sample_cascade": 2}), ("plain", {"filter": 1, "sample_cascade": 0}), ("scan", {"filter": 0})):
        for key, value in options.items():
            ix.set_option(key, value)
        before = {key: ix.stat(key) for key in ("cascade_passes", "i8v2_passes", "scan_launches", "fallback_queries")}
        dist, rows = ix.search(q, k)
        moved = {key: ix.stat(key) - before[key] for key in before}
        if name == "cascade":
            assert moved["cascade_passes"] == int(cascade), (name, moved)
            if cascade:
                assert ix.stat("last_cascade_d") == d
        else:
            assert moved["cascade_passes"] == 0, (name, moved)
        if name == "scan":
            assert moved["i8v2_passes"] == 0 and moved["scan_launches"] >= 1, moved
        out[name] = (dist.copy(), rows.copy(), moved, ix.last_pass(keys_per_query=keys_per_query, want_bmeta=False) if name == "cascade" and cascade else None)
    ix.set_option("filter", 1)
    ix.set_option("sample_cascade", 2)
    for name in ("cascade", "plain"):
        assert np.array_equal(out[name][1], out["scan"][1]), name
        assert np.array_equal(out[name][0].view(np.uint32), out["scan"][0].view(np.uint32)), name
    return out["cascade"]


N_RAGGED = TILE_ROWS * (D + 1) * 3 + 37      # 100 tiles: A1 = {0, 33, 66, 99}, a ragged last tile that is one of A1's
N_ONE_ROUND = TILE_ROWS * 256 + 5            # 257 tiles on 256 compute units: 249 tiles for B, one per workgroup, seven workgroups without
N_ROUNDS = 600_077                           # 2,345 tiles: 72 for A1, 2,273 for B — nine rounds, the last one ragged
SIZES = {"ragged": N_RAGGED, "one_round": N_ONE_ROUND, "rounds": N_ROUNDS}


@pytest.fixture(scope="module")
def corpora(Index, torch_):
    made = {}

    def get(name):
        if name not in made:
            made[name] = new_index(Index, torch_, SIZES[name], 1000 + len(name))
        return made[name]

    yield get
    for ix in made.values():
        ix.close()


# k = 64 needs a first sample of 128 tiles: tiles 1, 4, 7, ... give 33 of 100 and 86 of 257, so only the largest corpus takes the cascade
# there (100 tiles: the filter itself does not apply — its sample must hold 2k tiles — and all three searches are the exact scan)
@pytest.mark.parametrize("name,k,cascade", [("ragged", 1, True), ("ragged", 10, True), ("ragged", 64, False),
                                            ("one_round", 1, True), ("one_round", 10, True), ("one_round", 64, False),
                                            ("rounds", 1, True), ("rounds", 10, True), ("rounds", 64, True)])
def test_row_counts(corpora, name, k, cascade):
    ix = corpora(name)
    assert ix.stat("num_cus") % D == 0, "these cases are laid out for a grid that 32 divides"
    n = SIZES[name]
    q = queries(256, n + k)
    near = ix.read_rows(n - 1, 1)[0, :DIM]
    q[9] = near + 0.02 * q[9]                    # a neighbour in the ragged last tile
    dist, rows, moved, lp = three_ways(ix, q, k, cascade)
    assert rows[9, 0] == n - 1
    if cascade:
        assert moved["fallback_queries"] == 0, "random data must not need the fallback"
        assert (lp["family"], lp["ts"], lp["cascade_d"]) == ("TILE", 3, D)
        tiles = [1 + u * lp["sample_stride"] for u in range(lp["sample_tiles"])]
        assert all(t % (D + 1) and t * TILE_ROWS < n for t in tiles) and len(tiles) >= 2 * k


def test_planted_rows(corpora):
    """near-duplicates of queries in tile 0, in another of A1's tiles, in the last tile and in one of A0's: each must come back first"""
    ix = corpora("rounds")
    n = N_ROUNDS
    q = queries(256, 77)
    ix.set_option("sample_cascade", 2)
    ix.search(q, 10)
    lp = ix.last_pass(keys_per_query=1, want_bmeta=False)
    assert lp["cascade_d"] == D
    a0_tile = 1 + 5 * lp["sample_stride"]
    planted = {0: 5, 1: 255, 2: (D + 1) * 7 * TILE_ROWS + 100, 3: (D + 1) * 71 * TILE_ROWS + 3, 4: n - 3, 5: n - 1, 6: a0_tile * TILE_ROWS + 17,
               7: TILE_ROWS + 1, 8: (D + 1) * TILE_ROWS - 1, 9: (D + 1) * TILE_ROWS + TILE_ROWS}
    for z, row in planted.items():
        q[z] = ix.read_rows(row, 1)[0, :DIM] + 0.01 * q[z]
    for k in (1, 10):
        dist, rows, moved, _ = three_ways(ix, q, k)
        for z, row in planted.items():
            assert rows[z, 0] == row, (k, z, row, rows[z, :3])


def test_tombstones_in_sampled_tiles(Index, torch_):
    """rows deleted inside A1's tiles, among them the best A1 candidate of some queries, inside an A0 tile and elsewhere"""
    n = N_ONE_ROUND
    ix = new_index(Index, torch_, n, 31)
    assert ix.stat("num_cus") % D == 0, "these cases are laid out for a grid that 32 divides"
    q = queries(256, 32)
    best = {0: 17, 1: (D + 1) * 3 * TILE_ROWS + 200, 2: (D + 1) * 7 * TILE_ROWS + 1, 3: 4 * TILE_ROWS + 9}   # (3: an A0 tile)
    for z, row in best.items():
        q[z] = ix.read_rows(row, 1)[0, :DIM] + 0.01 * q[z]
    dist, rows, _, _ = three_ways(ix, q, 10)
    assert [rows[z, 0] for z in best] == list(best.values())
    rng = np.random.default_rng(33)
    a1_rows = np.concatenate([np.arange(t * TILE_ROWS, min(n, (t + 1) * TILE_ROWS)) for t in range(0, (n + TILE_ROWS - 1) // TILE_ROWS, D + 1)])
    dead = np.unique(np.concatenate([np.array(list(best.values())), rng.choice(a1_rows, 600, replace=False), rng.choice(n, 300, replace=False),
                                     rows[:40, 0]]))   # ... and the first neighbour of 40 queries, wherever it lies
    ix.delete(dead)
    dist2, rows2, _, _ = three_ways(ix, q, 10)
    assert not np.isin(rows2, dead).any()
    assert not np.array_equal(rows2[:40], rows[:40])
    ix.close()


def test_fewer_than_k_candidates_from_the_sampled_tiles(Index, torch_):
    """A1's tiles hold only never-written zero rows: no query with a positive threshold gets a candidate from them, so the re-anchor's
    k rows come from A0's keys alone; a zero query (every row scores 0) sees them all"""
    n = N_ONE_ROUND - 5
    tiles = n // TILE_ROWS
    ranges = [(t * TILE_ROWS, min(tiles, t + D) * TILE_ROWS) for t in range(1, tiles, D + 1)]
    ix = new_index(Index, torch_, ranges[-1][1], 41, ranges)
    assert ix.stat("num_cus") % D == 0, "these cases are laid out for a grid that 32 divides"
    q = queries(256, 42)
    q[11] = 0.0
    dist, rows, moved, lp = three_ways(ix, q, 10, keys_per_query=4096)
    assert lp["cascade_d"] == D
    in_a1 = [int(np.sum((fs.key_rows(keys) // TILE_ROWS) % (D + 1) == 0)) for keys in lp["keys"][:10]]
    assert in_a1 == [0] * 10 and all(len(keys) >= 10 for keys in lp["keys"][:10]), in_a1
    ix.close()


def test_candidate_counts_are_deterministic(corpora):
    ix = corpora("one_round")
    q = queries(256, 55)
    ix.set_option("sample_cascade", 2)
    seen = set()
    for _ in range(10):
        before = (ix.stat("filter_hits"), ix.stat("filter_survivors"), ix.stat("cascade_passes"))
        ix.search(q, 10)
        seen.add((ix.stat("filter_hits") - before[0], ix.stat("filter_survivors") - before[1], ix.stat("cascade_passes") - before[2]))
    assert len(seen) == 1, seen
    hits, survivors, passes = next(iter(seen))
    assert passes == 1 and hits >= 256 * 10 and survivors >= 256 * 10


@pytest.mark.parametrize("B,nbq,options", [(130, 8, {}), (100, 4, {"resident_q": 0})])
def test_other_batches(corpora, B, nbq, options):
    """130 queries (the smallest batches of the 16-query-block instantiation) and 100 (65..128 queries: the 8-query-block one, which
    runs the static program once "resident_q" = 0 takes the resident one away)"""
    ix = corpora("one_round")
    for key, value in options.items():
        ix.set_option(key, value)
    try:
        dist, rows, moved, lp = three_ways(ix, queries(B, 66 + B), 10)
    finally:
        for key in options:
            ix.set_option(key, 1)
    assert (lp["nq"], lp["nbq"], lp["ts"], lp["res"], lp["cascade_d"]) == (B, nbq, 3, 0, D)


def test_the_size_rule_leaves_a_small_index_alone(corpora):
    ix = corpora("one_round")
    q = queries(256, 88)
    ix.set_option("sample_cascade", 1)
    before = ix.stat("cascade_passes")
    d1, r1 = ix.search(q, 10)
    assert ix.stat("cascade_passes") == before and ix.stat("last_cascade_d") == 0 and ix.last_pass(keys_per_query=1, want_bmeta=False)["cascade_d"] == 0
    ix.set_option("sample_cascade", 2)
    d2, r2 = ix.search(q, 10)
    assert ix.stat("cascade_passes") == before + 1
    assert np.array_equal(r1, r2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


def test_default_d(corpora):
    """the shipped "cascade_d" = 16: A1 is every 17th tile, launch B's step is 272, A0's stride a multiple of 17"""
    ix = corpora("rounds")
    q = queries(256, 99)
    q[0] = ix.read_rows(17 * 5 * TILE_ROWS + 9, 1)[0, :DIM] + 0.01 * q[0]     # a neighbour in one of A1's tiles
    q[1] = ix.read_rows(N_ROUNDS - 2, 1)[0, :DIM] + 0.01 * q[1]               # ... and in the last tile
    ix.set_option("cascade_d", 16)
    try:
        dist, rows, moved, lp = three_ways(ix, q, 10, d=16)
    finally:
        ix.set_option("cascade_d", D)
    assert (rows[0, 0], rows[1, 0]) == (17 * 5 * TILE_ROWS + 9, N_ROUNDS - 2)
    assert lp["cascade_d"] == 16 and lp["sample_stride"] % 17 == 0 and lp["sample_tiles"] >= 20 and moved["fallback_queries"] == 0


@pytest.mark.parametrize("sample_tiles,cascade", [(40, True), (16, False)])
def test_first_sample_obeys_sample_tiles(Index, torch_, sample_tiles, cascade):
    """"sample_tiles" sizes the sample's key buffer: the first sample takes no more tiles than that (40), and where that is fewer than 2k
    (16) there is no cascade — nor a filter pass: the plain sample is cut to 16 tiles as well and the search is the exact scan"""
    ix = new_index(Index, torch_, N_ONE_ROUND, 51)
    ix.set_option("sample_tiles", sample_tiles)
    dist, rows, moved, lp = three_ways(ix, queries(256, 52), 10, cascade)
    if cascade:
        assert lp["sample_tiles"] == sample_tiles and lp["cascade_d"] == D
    else:
        assert moved["i8v2_passes"] == 0
    ix.close()
