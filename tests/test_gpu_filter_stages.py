"""What each stage of a filter pass hands on: the sample's bucket keys, the anchor's thresholds, the filter's candidate
lists — read back after a search (DeviceKnnIndex.last_pass, codd_knn_debug_last_pass) and held against the CPU reference of
tests/_filter_stage_reference.py, for every program filter_program() can choose.  The final top-k cannot see a lost candidate unless
the lost row is one of the k best; the rows that decide whether a cut is right sit at the threshold and never are.

Every case first asserts that the program that ran is the one its id names (a dispatch change must not move a test off the program
it was written for), then that the answer is the oracle's, then:

  sample      int8: every (query, sampled tile) key equals the reference's bit for bit.  2-byte: the score lies within ACC = dpad 2^-23
              (the fp32 accumulation order) of the tile's largest reference score, the row is a row of that tile whose reference score
              lies within 2 ACC of it.
  thresholds  thr (and thr0 on int8 operands) have the bits of fp32(L - eps) with L the smallest canonical exact score among the live
              rows of the k best DUMPED keys; and, independent of everything internal, L(q) <= the oracle's k-th best exact score.
  candidates  no row twice, none >= n, none for a padding query; every key's score is the reference's (int8: the bits; 2-byte: within
              ACC); every live row whose canonical exact score reaches L(q) is there (what |s~ - s| <= eps promises, no tolerance);
              and the cut itself:
                GEMM, int8    the list is exactly {row < n : fp32(acc s_row) >= fp32(thr / s_q)} — the rows with s~ >= thr (the same
                              rows, tests/test_filter_stage_bands.py); l2: {!(fma(acc s_row, 2 s_q, -|c|^2) < thr + |q|^2)}
                TILE, pb = 0  the list holds that set; every other row's accumulator is at most three levels below the smallest one
                              whose float score reaches thr: the kernel tests acc >= (int)(th / scale) - 2, the cast truncates
                TILE          m = acc scale_b s_q + B(q) e_b - thr0(q) in fp64 from the dumped scales: m > delta must be there,
                              m < -delta - 3 scale_b s_q must not, with
                                  delta = 8 * 2^-24 (|thr0| + B e_b)
                              for the fp32 roundings between the real-number margin and the kernel's integer threshold: th = thr0 / s_q
                              (1), u = B / s_q (1), u e_b (1), th - u e_b (1, of a difference no larger than |th| + u e_b), 1 / scale_b (1),
                              the product with it (1) — six relative 2^-24 of quantities no larger than (|thr0| + B e_b) / (s_q scale_b)
                              in accumulator units — and the pre-test's single fma against the threshold truncated to bf16 (1, and the
                              truncation only lowers it): eight covers them.  |thr0| < 1, B ~ 1, e_b ~ 0.01: delta ~ 5e-7.  The three
                              levels are the - 2 and the truncation, as above.
                2-byte        score > thr + ACC must be there, score < thr - ACC must not.
              Rows inside a band are exempt; a case counts only while they are at most 1 % of its candidates and 8 of one query.
"""

import dataclasses

import numpy as np
import pytest

from codd_query_engine_amd import native
from oracle import knn_oracle as o
from tests import _filter_stage_reference as fs

pytestmark = pytest.mark.gpu
K = fs.K


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def shadow_type():
    return "f16" if "shadow=f16" in native.load().codd_knn_version().decode() else "bf16"


def num_cus(Index):
    ix = Index(64)
    try:
        return ix.stat("num_cus")
    finally:
        ix.close()


def open_index(Index, case, raw, **options):
    ix = Index(raw.shape[1], dtype=case.dtype, space=case.space)
    for key, value in {**fs.BASE_OPTIONS, **case.options, **options}.items():
        ix.set_option(key, value)
    ix.upsert(np.arange(raw.shape[0], dtype=np.int64), raw, normalize=case.space == "cosine")
    return ix


def assert_answer(p, dist, rows, queries=None):
    """ids and distance bits are the oracle's, over the live rows"""
    dist, rows = np.asarray(dist), np.asarray(rows)
    for q in range(p.B) if queries is None else queries:
        score, want = p.topk(q, K)
        assert np.array_equal(rows[q], want), (q, rows[q], want)
        one = np.float32(0.0 if p.space == "l2" else 1.0)
        assert np.array_equal(fs.bits(dist[q]), fs.bits(one - score)), q


check_sample, check_thresholds, check_candidates = fs.check_sample, fs.check_thresholds, fs.check_candidates


def run_case(Index, case, raw, q, dead=None, **options):
    """build, search once, read the pass back; assert the program and the answer; returns (index, read-back, reference, answer)"""
    ix = open_index(Index, case, raw, **options)
    if dead is not None:
        ix.delete(np.flatnonzero(dead).astype(np.int64))
    stored = ix.read_rows()
    assert np.array_equal(stored, fs.stored_rows(case.space, raw, case.dtype))
    p = fs.Pass(case, stored, q, shadow_type(), dead)
    before = {key: ix.stat(key) for key in ("filter_passes", "i8v2_passes", "f16_tile_passes", "shadow8_passes")}
    dist, rows = ix.search(q, K)
    lp = ix.last_pass()
    ran = {key: lp[key] for key in case.program()}
    assert ran == case.program(), ("another program ran", ran)
    assert (lp["nq"], lp["k"], lp["n"]) == (p.B, K, p.n)
    ntiles = (p.n + fs.TILE - 1) // fs.TILE
    assert (lp["sample_tiles"], lp["sample_stride"]) == fs.sample_geometry(ntiles, K, bool(case.el), case.nbq, ix.stat("num_cus")), \
        "the device-free band test describes another sample than the one that ran"
    assert lp["per_block_filter"] == int(case.per_block)
    assert ix.stat("filter_passes") - before["filter_passes"] == 1
    assert ix.stat("i8v2_passes") - before["i8v2_passes"] == int(case.family == "TILE")
    assert ix.stat("f16_tile_passes") - before["f16_tile_passes"] == int(case.family == "TILE_F16")
    assert ix.stat("shadow8_passes") - before["shadow8_passes"] == case.el
    assert_answer(p, dist, rows)
    if case.space == "cosine" and dead is None:
        d_ref, i_ref = o.search(stored, case.dtype, p.Q, K)
        assert np.array_equal(rows, i_ref) and np.array_equal(dist, d_ref)
    return ix, lp, p, (dist, rows)


@pytest.fixture(scope="module")
def cus(Index):
    return num_cus(Index)


@pytest.mark.parametrize("case", fs.CASES, ids=lambda c: c.id)
def test_stage_products(Index, cus, case):
    raw, q = fs.make_data(case, cus)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    try:
        if case.multi:
            ntiles = (p.n + 255) // 256
            assert ntiles > 2 * cus and ntiles < 3 * cus, "workgroups of two and of three tiles"
        assert lp["fb_count"] == 0 and lp["flags"][1] == 0 and ix.stat("fallback_queries") == 0
        print(case.id, "ran", {key: lp[key] for key in case.program()}, "n", lp["n"], "cus", cus, "sampled", lp["sample_tiles"], "stride",
              lp["sample_stride"], "counters", int(lp["hit_counts"].astype(np.int64).sum()), "thr", float(lp["thr"][: p.B].min()),
              float(lp["thr"][: p.B].max()), "eps16", lp["eps"])
        check_sample(p, lp)
        L, thr, thr0 = check_thresholds(p, lp)
        cand = check_candidates(p, lp, L, thr, thr0)
        print(case.id, "reference candidates", cand)
        assert cand >= 10 * p.B
    finally:
        ix.close()


def test_read_back_without_a_pass_is_an_argument_error(Index):
    """EINVAL, nothing copied, for a stream no filter pass has run on: before any search, and after one the exact scan answered"""
    rng = np.random.default_rng(1)
    raw = rng.standard_normal((600, 64)).astype(np.float32)
    ix = Index(64)
    ix.upsert(np.arange(600, dtype=np.int64), raw)
    with pytest.raises(native.NativeLibraryError, match="no filter pass"):
        ix.last_pass()
    ix.search(raw[:3], 5)                     # 3 tiles: the exact scan
    assert ix.stat("filter_passes") == 0
    with pytest.raises(native.NativeLibraryError, match="no filter pass"):
        ix.last_pass()
    assert ix.stat("workspaces") == 1         # (the failed read-backs took no workspace of their own)
    ix.close()


def test_read_back_changes_nothing_and_takes_caps(Index):
    case = fs.CASE_BY_ID["gemm8-res1-nbq2"]
    raw, q = fs.make_data(case)
    ix, lp, p, (dist, rows) = run_case(Index, case, raw, q)
    again = ix.last_pass()
    for key in ("thr", "thr0", "qmeta", "hit_counts", "bucket_max", "bmeta"):
        assert np.array_equal(lp[key].view(np.uint32), again[key].view(np.uint32)), key
    capped = ix.last_pass(keys_per_query=3)
    assert all(np.array_equal(capped["keys"][i], lp["keys"][i][:3]) for i in range(256))
    import ctypes

    small = np.zeros(4, dtype=np.uint64)
    rc = ix._lib.codd_knn_debug_last_pass(ix._h, ix._stream(), None, None, None, None, None, None, 0, small.ctypes.data_as(ctypes.c_void_p), 4, None, 0)
    assert rc == -22 and not small.any()
    d2, r2 = ix.search(q, K)
    assert np.array_equal(r2, rows) and np.array_equal(fs.bits(d2), fs.bits(dist))
    ix.close()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
# each on the static tile program (768 elements, 16 query blocks) and on the staged int8 GEMM (2 query blocks: finalize and the
# fallback queue are launches of their own there; the tile program's batch takes the fused finalize)

EDGE_PROGRAMS = {"tile-static": "tile-staged-ts3-d768-nbq8", "gemm8-staged": "gemm8-staged-nbq2"}
edge_programs = pytest.mark.parametrize("program", list(EDGE_PROGRAMS))


def edge(program, **changes):
    base = fs.CASE_BY_ID[EDGE_PROGRAMS[program]]
    return dataclasses.replace(base, id=f"edge-{program}", options={**base.options, **changes.pop("options", {})}, **changes)


def check_all(ix, lp, p, **kw):
    check_sample(p, lp)
    L, thr, thr0 = check_thresholds(p, lp)
    check_candidates(p, lp, L, thr, thr0, **kw)
    return L, thr, thr0


def rows_of(lp, q):
    return set(fs.key_rows(lp["keys"][q]).tolist())


@edge_programs
def test_negated_row_gives_thresholds_below_zero(Index, program):
    """Rows that share a component, and a query that is the negation of one of them: every score of that query is negative, so are
    its thresholds, and the tile kernel's bf16 pre-test (conclusive for positive thresholds only) must hand every block pair to the
    per-value test."""
    case = edge(program, seed=101)
    raw, q = fs.make_data(case)
    rng = np.random.default_rng(101)
    v = rng.standard_normal(case.d).astype(np.float32)
    raw += np.float32(0.5) * v * np.float32(np.sqrt(case.d)) / np.linalg.norm(v)
    q[8] = -raw[11]
    ix, lp, p, _ = run_case(Index, case, raw, q)
    L, thr, thr0 = check_all(ix, lp, p)
    assert L[8] < 0 and lp["thr"][8] < 0 and (case.family != "TILE" or lp["thr0"][8] < 0)
    assert len(lp["keys"][8]) >= K and lp["fb_count"] == 0 and ix.stat("fallback_queries") == 0
    ix.close()


@edge_programs
def test_zero_and_nan_queries_keep_every_row(Index, program):
    """A zero query, and one with a NaN element (prepared as the zero query): scale 0, every approximate score 0, L = 0 and a threshold
    below zero, which the kernels divide by the scale: -inf, every row below n a candidate with score 0.  No counter is poisoned, no
    flag set, nothing queued: finalize re-scores the n rows and answers with the oracle's k lowest rows."""
    case = edge(program, seed=102)
    raw, q = fs.make_data(case)
    q[7] = 0.0
    q[9, 3] = np.nan
    ix, lp, p, (dist, rows) = run_case(Index, case, raw, q)
    L, thr, thr0 = check_all(ix, lp, p)
    for z in (7, 9):
        assert lp["qmeta"][z] == 0.0 and L[z] == 0.0 and lp["thr"][z] < 0
        assert lp["hit_counts"][z] == p.n and rows_of(lp, z) == set(range(p.n))
        assert not fs.key_scores(lp["keys"][z]).any()
        assert np.array_equal(rows[z], np.arange(K))
    assert lp["fb_count"] == 0 and lp["flags"][1] == 0 and ix.stat("fallback_queries") == 0
    ix.close()


@edge_programs
def test_duplicated_blocks_within_and_across_tiles(Index, program):
    """One 32-row block stored three times — twice in tile 0, once in tile 1 (whole blocks: an int8 block has one scale, so the copies
    quantise alike): equal approximate scores, all copies among the candidates, the sample key of tile 0 names the lower row."""
    case = edge(program, seed=103)
    raw, q = fs.make_data(case)
    raw[32:64] = raw[0:32]
    raw[256:288] = raw[0:32]
    rng = np.random.default_rng(103)
    q[4] = raw[7] + np.float32(0.02) * rng.standard_normal(case.d).astype(np.float32)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    check_all(ix, lp, p)
    keys = {int(r): k for r, k in zip(fs.key_rows(lp["keys"][4]), lp["keys"][4])}
    assert {7, 39, 263} <= set(keys)
    assert len({int(keys[r]) >> 32 for r in (7, 39, 263)}) == 1, "the copies' approximate scores differ"
    assert fs.key_rows(lp["bucket_max"][4, :2]).tolist() == [7, 263]
    ix.close()


@edge_programs
def test_a_block_of_near_copies_of_one_query(Index, program):
    """32 near-copies of one query in one 32-row block: every lane of the tile kernel's epilogue holds several hits among its 8 rows
    (the cnt > 1 path appends them one by one).  All 32 are there, once each."""
    case = edge(program, seed=104)
    raw, q = fs.make_data(case)
    rng = np.random.default_rng(104)
    raw[64:96] = q[2] + np.float32(0.01) * rng.standard_normal((32, case.d)).astype(np.float32)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    check_all(ix, lp, p)
    got = fs.key_rows(lp["keys"][2])
    assert set(range(64, 96)) <= set(got.tolist()) and len(set(got.tolist())) == len(got)
    ix.close()


def dense_tile(case, seed):
    """tile 10 is 256 near-copies of one vector that four queries in five point at"""
    raw, q = fs.make_data(case)
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(case.d).astype(np.float32)
    raw[2560:2816] = centre + np.float32(1e-3) * rng.standard_normal((256, case.d)).astype(np.float32)
    pointing = case.B * 4 // 5
    q[:pointing] = centre + np.float32(1e-3) * rng.standard_normal((pointing, case.d)).astype(np.float32)
    return raw, q, pointing


@edge_programs
def test_one_dense_tile_fills_the_workgroup_list(Index, program):
    """256 near-copies in one tile, 160 (40) queries pointing at them: 40,960 (10,240) hits inside one tile, more than the workgroup's
    LDS list holds (4,096 entries at most) — the rest is appended to the queries' global lists directly.  That it happened: all hits
    of a tile come from one workgroup, and the read-back counts more than 4,096 in tile 10; the tile kernel also sets its statistics
    flag (gemm_filter_kernel's never fires for a tile: its flush at the tile's end empties the list before the flag is looked at).
    The lists are complete and hold no row twice."""
    case = edge(program, seed=105)
    raw, q, pointing = dense_tile(case, 105)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    check_all(ix, lp, p)
    in_tile = sum(int(((fs.key_rows(lp["keys"][z]) >= 2560) & (fs.key_rows(lp["keys"][z]) < 2816)).sum()) for z in range(p.B))
    assert in_tile > 4096, "the workgroup list did not fill: the case tests nothing"
    assert lp["flags"][0] == int(case.family == "TILE")
    for z in range(pointing):
        assert set(range(2560, 2816)) <= rows_of(lp, z)
    assert lp["fb_count"] == 0 and ix.stat("fallback_queries") == 0
    ix.close()


@edge_programs
def test_hit_cap_below_a_querys_candidates(Index, program):
    """The same data with "hit_cap" = 128: the pointing queries' raw counters pass the cap, they are answered by the exact-scan
    fallback (the fused finalize of the large batch derives the queue from the counters: flag and stat; the small batch's finalize
    writes the queue: fb_list), the other queries' lists are complete, every answer is exact (run_case)."""
    case = edge(program, seed=105, options={"hit_cap": 128})
    raw, q, pointing = dense_tile(case, 105)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    over = set(np.flatnonzero(lp["hit_counts"].astype(np.int64) > 128).tolist())
    assert set(range(pointing)) <= over and lp["hit_cap"] == 128
    assert all(len(lp["keys"][z]) == 128 for z in over)
    check_sample(p, lp)
    L, thr, thr0 = check_thresholds(p, lp)
    check_candidates(p, lp, L, thr, thr0, skip=over)
    assert lp["flags"][1] == 1 and ix.stat("fallback_queries") == len(over)
    if p.B <= 64:      # finalize as its own launch: the queue is written
        assert lp["fb_count"] == len(over) and set(lp["fb_list"][: len(over)].tolist()) == over
    ix.close()


def test_a_spread_cluster_flushes_the_static_programs_list_repeatedly(Index, cus):
    """The 30,000-member cluster of tests/test_gpu_i8_tile.py scaled down: 3,500 near-copies spread over all 515 tiles (two or three
    tiles per workgroup), 200 queries pointing at them.  A workgroup empties its LDS list at the first tile end with more than
    kHitCap / 2 = 1,024 entries; the candidates of the read-back, counted per tile, show workgroups whose first AND second tile each
    exceed that on their own — two flushes inside the loop and the one at the end.  The soundness statement is taken for every 16th
    query (3,500 canonical scores each), every other statement for all."""
    case = dataclasses.replace(fs.CASE_BY_ID["multi-tile-ts3"], id="edge-flush", B=256, seed=106)
    raw, q = fs.make_data(case, cus)
    n = raw.shape[0]
    rng = np.random.default_rng(106)
    centre = rng.standard_normal(case.d).astype(np.float32)
    centre /= np.linalg.norm(centre)
    members = rng.choice(n, size=3_500, replace=False)
    spread = np.float32(0.12 / np.sqrt(case.d))
    raw[members] = centre + spread * rng.standard_normal((3_500, case.d)).astype(np.float32)
    q[:200] = centre + spread * rng.standard_normal((200, case.d)).astype(np.float32)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    check_sample(p, lp)
    L, thr, thr0 = check_thresholds(p, lp)
    check_candidates(p, lp, L, thr, thr0, sound=range(0, 256, 16))
    per_tile = np.zeros((n + 255) // 256, dtype=np.int64)
    for z in range(256):
        np.add.at(per_tile, fs.key_rows(lp["keys"][z]) // 256, 1)
    G = min(cus, len(per_tile))
    twice = [b for b in range(G) if b + G < len(per_tile) and per_tile[b] > 1024 and per_tile[b + G] > 1024]
    print("workgroups whose first two tiles each pass the flush mark:", len(twice), "of", G, "largest tile:", per_tile.max())
    assert len(twice) >= G // 4
    assert ix.stat("fallback_queries") == 0
    ix.close()


@edge_programs
def test_tombstones(Index, program):
    """Deleted rows: two queries' nearest rows, a third of tile 2, and all of tile 5 but one row.  The filter kernels do not look at
    tombstones — dead rows still appear among the candidates — but L comes from live anchors only and the
    soundness statement is taken over the live rows."""
    case = edge(program, seed=107)
    raw, q = fs.make_data(case)
    dead = np.zeros(raw.shape[0], dtype=bool)
    dead[[0, raw.shape[0] // 2]] = True
    dead[512:768:3] = True
    dead[1280:1535] = True
    ix, lp, p, (dist, rows) = run_case(Index, case, raw, q, dead=dead)
    check_all(ix, lp, p)
    assert not dead[rows[: p.B]].any()
    assert any(dead[fs.key_rows(lp["keys"][z])].any() for z in range(p.B)), "no dead row among the candidates: the case tests nothing"
    assert raw.shape[0] // 2 in rows_of(lp, 3) and 0 in rows_of(lp, 6)
    ix.close()


@edge_programs
def test_second_search_on_the_same_workspace_starts_clean(Index, program):
    """Two searches in a row with different queries, the second batch smaller: its read-back holds its own candidates only — the
    counters of the queries that are padding now are zero, no list holds a row of the first search that the second's cut drops."""
    case = edge(program, seed=108)
    raw, q = fs.make_data(case)
    ix, lp, p, _ = run_case(Index, case, raw, q)
    check_all(ix, lp, p)
    smaller = {200: 140, 50: 40}[case.B]
    case2 = dataclasses.replace(case, B=smaller, seed=109)
    _, q2 = fs.make_data(case2)
    p2 = fs.Pass(case2, ix.read_rows(), q2, shadow_type())
    dist, rows = ix.search(q2, K)
    lp2 = ix.last_pass()
    assert {key: lp2[key] for key in case2.program()} == case2.program() and lp2["nq"] == smaller
    assert_answer(p2, dist, rows)
    check_all(ix, lp2, p2)
    assert not lp2["hit_counts"][smaller:].any()
    ix.close()
