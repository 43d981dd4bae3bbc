"""Write sequences: gaps past the count, compaction followed by writes, partial shadow rebuilds.

A search answer comes from up to four copies of a row: the stored row, the int8 shadow, the 2-byte shadow, and the int8 meta data
(`rscale` per row, `bmeta` per 32-row block).  The tests that write once and search cannot see one of them going stale, and random
data hides a stale shadow behind the filters' slack.  Here every index is written several times, and the queries are chosen so
that a stale copy changes the answer:

    -e0       every written row has a clearly positive first component (raw rows are standard_normal + 8 e0), so it scores below 0;
              a never-written slot is the zero vector, scores exactly 0, and the k lowest such slots ARE the answer
    ghosts    the raw vectors of rows that were deleted and whose old slots are never-written slots again after the compaction:
              whatever still holds the old row answers with that slot at distance ~0

The model is DeletingOracleEngine (the CPU oracle over the live rows, never-written slots as zero rows).  Every comparison is bit
for bit on rows and distances.  The paths are chosen by option on one index; each proves itself by the stat that must move (and
the one that must not)."""

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests import _space_reference as sr
from tests._deleting_oracle_engine import DeletingOracleEngine
from tests._int8_reference import int8_scores, quantise_like_the_kernels, row_error_norms
from tests._space_oracle_engine import SpaceOracleEngine

pytestmark = pytest.mark.gpu

DIM, K = 384, 10      # three int8 K-steps (the least i8_tile_kernel takes), six 64-element K-steps (an f16-tile width)

# name: queries, options, the stat that must move, the stat that must not
PATHS = {
    "scan": (8, {"filter": 0}, "scan_launches", "filter_passes"),
    "i8_gen1": (20, {"i8v2": 0}, "shadow8_passes", "i8v2_passes"),
    "i8_tile": (140, {}, "i8v2_passes", "f16_tile_passes"),
    "gemm16": (40, {"shadow8": 0, "f16_tile": 0}, "filter_passes", "shadow8_passes"),
    "f16_tile": (140, {"shadow8": 0}, "f16_tile_passes", "shadow8_passes"),
    "mask_list": (8, {"mask_route": 1}, "mask_list_searches", None),
}
DEFAULTS = {"filter": 1, "i8v2": 2, "shadow8": 1, "f16_tile": 1, "mask_route": 0}
FILTERS = ["i8_gen1", "i8_tile", "gemm16", "f16_tile", "mask_list"]
EVERY_PATH = ["scan"] + FILTERS
WRITERS = ["upsert", "upsert_device", "load_rows"]


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return torch, DeviceKnnIndex


def rows_like(rng, n):
    raw = rng.standard_normal((n, DIM)).astype(np.float32)
    raw[:, 0] += 8.0
    return raw


def query_batch(rng, special=()):
    """140 queries: -e0, then `special` (ghosts, rows just written), then random ones.  The special ones sit in front of the
    smallest batch any path takes."""
    q = rng.standard_normal((140, DIM)).astype(np.float32)
    q[0] = 0.0
    q[0, 0] = -1.0
    assert len(special) <= 7
    for j, v in enumerate(special):
        q[1 + j] = v
    return q


def always_filter(ix):
    for key in ("filter_min_rows", "filter_min_rows_small", "filter_min_batch"):
        ix.set_option(key, 1)
    ix.set_option("shadow8_cooldown", 0)


def make(env, dtype="f32", space="cosine"):
    _, Index = env
    ix = Index(DIM, dtype=dtype, space=space)
    model = DeletingOracleEngine(DIM, dtype) if space == "cosine" else SpaceOracleEngine(DIM, dtype, space)
    return ix, model


def storage_rows(model, raw):
    """raw vectors as the model's index stores them (what load_rows takes)"""
    if getattr(model, "space", "cosine") == "cosine":
        return o.to_storage(o.normalize_rows(raw), model.dtype)
    return sr.stored(raw, model.dtype)


def write(env, ix, model, writer, first, raw):
    """`raw` into slots [first, first + n) of the index and of the model.  upsert_device writes on a side stream that nobody
    synchronises: the searches that follow run on the default stream and have to wait for it on the device.  Returns what has
    to stay alive until then."""
    torch, _ = env
    slots = np.arange(first, first + raw.shape[0], dtype=np.int64)
    normalize = getattr(model, "space", "cosine") == "cosine"
    if writer == "load_rows":
        rows = storage_rows(model, raw)
        ix.load_rows(rows, first_slot=first)
        model.load_rows(rows, first_slot=first)
        return None
    model.upsert(slots, raw, normalize)
    if writer == "upsert":
        ix.upsert(slots, raw, normalize)
        return None
    assert writer == "upsert_device"
    dev = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ix.upsert_device(first, dev, normalize)
    dev.record_stream(side)
    return dev


def run_path(ix, name, q):
    B, options, moved, still = PATHS[name]
    for key, value in options.items():
        ix.set_option(key, value)
    before, frozen = ix.stat(moved), ix.stat(still) if still else 0
    try:
        if name == "mask_list":
            dist, rows = ix.search_masked(q[:B], np.ones(ix.count(), dtype=bool), K)
        else:
            dist, rows = ix.search(q[:B], K)
    finally:
        for key in options:
            ix.set_option(key, DEFAULTS[key])
    assert ix.stat(moved) > before, (name, moved, "did not move")
    assert not still or ix.stat(still) == frozen, (name, still, "moved")
    return dist, rows


def reference(model, q, names):
    B = max(PATHS[name][0] for name in names)
    return model.search(q[:B], K)


def compare(ix, ref, q, names, what):
    """every path of `names` against the model's answer; all the paths are run, then the differences are reported together"""
    d_ref, r_ref = ref
    wrong = []
    for name in names:
        B = PATHS[name][0]
        dist, rows = run_path(ix, name, q)
        bad = np.flatnonzero((rows != r_ref[:B]).any(axis=1))
        if bad.size:
            b = int(bad[0])
            wrong.append(f"{what}: {name}: rows differ for queries {bad[:6].tolist()}; query {b} got {rows[b].tolist()} want {r_ref[b].tolist()}")
        elif not np.array_equal(dist, d_ref[:B]):
            b = int(np.flatnonzero((dist != d_ref[:B]).any(axis=1))[0])
            wrong.append(f"{what}: {name}: distances differ; query {b} got {dist[b].tolist()} want {d_ref[b].tolist()}")
    assert not wrong, "\n" + "\n".join(wrong)


def zero_slots_answer_minus_e0(ref, unwritten):
    """precondition, from the reference alone: query 0 (-e0) is answered by the k lowest live never-written slots at distance 1"""
    d_ref, r_ref = ref
    assert np.array_equal(r_ref[0], unwritten[:K]) and (np.diff(r_ref[0]) > 0).all(), (r_ref[0], unwritten[:K])
    assert (d_ref[0] == np.float32(1.0)).all(), d_ref[0]


def ghosts_are_gone(ref, ghost_slots):
    """precondition, from the reference alone: the answer to ghost query j (query 1 + j) does not hold the ghost's old slot"""
    for j, slot in enumerate(ghost_slots):
        assert slot not in ref[1][1 + j].tolist(), (slot, ref[1][1 + j])


def assert_zero_rows(ix, first, n):
    assert n > 0 and not ix.read_rows(first, n).any(), f"slots [{first}, {first + n}) were never written: zero rows"


# ------------------------------------------------------------------------------------------------------------------------
# (a) a gap inside the shadows' head room
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("writer", WRITERS)
def test_gap_inside_the_shadows_head_room(env, writer):
    """8,192 rows, searched on every path: both shadows exist, each allocated for 9,216 rows.  A write of [8,800, 8,900) stays
    inside them and leaves [8,192, 8,800) never written: zero rows in the row store, and both shadows and the int8 meta data
    have to say so too."""
    rng = np.random.default_rng(100 + WRITERS.index(writer))
    n, first, m = 8192, 8800, 100
    ix, model = make(env)
    raw = rows_like(rng, n)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    model.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)
    q = query_batch(rng)
    compare(ix, reference(model, q, EVERY_PATH), q, EVERY_PATH, "built")
    assert ix.stat("shadow8_builds") >= 1 and ix.stat("shadow16_builds") >= 1

    keep = write(env, ix, model, writer, first, rows_like(rng, m))
    assert ix.count() == model.count() == first + m
    gap = np.arange(n, first)
    ref = reference(model, q, EVERY_PATH)
    zero_slots_answer_minus_e0(ref, gap)
    compare(ix, ref, q, EVERY_PATH, f"gap write by {writer}")
    assert_zero_rows(ix, n, first - n)
    del keep

    dead = np.array([n, n + 1, n + 5], dtype=np.int64)           # never-written slots are live rows: deletable
    ix.delete(dead)
    model.delete(dead)
    assert ix.live_count() == model.live_count() == first + m - 3
    ref = reference(model, q, EVERY_PATH)
    zero_slots_answer_minus_e0(ref, np.setdiff1d(gap, dead))
    compare(ix, ref, q, EVERY_PATH, "three gap slots deleted")
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# (b), (c) a gap after compaction, the row store not regrown: the vacated slots still held the deleted rows
# ------------------------------------------------------------------------------------------------------------------------
GHOSTS = [6300, 6600, 6950]     # deleted with [6,144, 8,192); below every first written slot, clear of the scattered write's 6,500


def ghost_scenario(env, seed, dtype, space, writer, consumed, names):
    rng = np.random.default_rng(seed)
    n = 8192
    ix, model = make(env, dtype, space)
    cosine = space == "cosine"
    ix.reserve(16384)                                             # no write below regrows the store (a regrow zeroes the new capacity)
    raw = rows_like(rng, n)
    ix.upsert(np.arange(n, dtype=np.int64), raw, cosine)
    model.upsert(np.arange(n, dtype=np.int64), raw, cosine)
    always_filter(ix)
    q = query_batch(rng, [raw[g] for g in GHOSTS])
    if cosine:                                                    # both shadows hold rows 0 .. 8,191 before anything is deleted
        for name in ("i8_tile", "gemm16"):
            run_path(ix, name, q)
        assert ix.stat("shadow8_builds") == 1 and ix.stat("shadow16_builds") == 1
    dead = np.concatenate([np.arange(6144, n), rng.permutation(6144)[:100]])
    ix.delete(dead)
    model.delete(dead)
    live = n - dead.size
    assert ix.compact() == model.compact() == live == 6044
    if consumed:                                                  # both dirty ranges are consumed: the next write dirties only what it says
        for name in ("i8_tile", "gemm16"):
            run_path(ix, name, q)
        assert ix.stat("shadow8_builds") == 2 and ix.stat("shadow16_builds") == 2
    if writer == "scattered":
        slots = np.array([6500, 7900], dtype=np.int64)
        vecs = rows_like(rng, 2)
        ix.upsert(slots, vecs, cosine)
        model.upsert(slots, vecs, cosine)
        keep, written = None, slots
    else:
        keep = write(env, ix, model, writer, 7000, rows_like(rng, 100))
        written = np.arange(7000, 7100)
    assert ix.count() == model.count() == written.max() + 1
    unwritten = np.setdiff1d(np.arange(live, written.max() + 1), written)
    assert np.isin(GHOSTS, unwritten).all()
    ref = reference(model, q, names)
    zero_slots_answer_minus_e0(ref, unwritten)
    ghosts_are_gone(ref, GHOSTS)
    compare(ix, ref, q, names, f"{dtype} {space}: gap write by {writer} after compaction, dirty ranges {'consumed' if consumed else 'pending'}")
    for lo, hi in ((live, 6500), (6501, 7900)) if writer == "scattered" else ((live, 7000),):
        assert_zero_rows(ix, lo, hi - lo)
    del keep
    ix.close()


@pytest.mark.parametrize("consumed", [True, False], ids=["consumed", "pending"])
@pytest.mark.parametrize("writer", WRITERS + ["scattered"])
def test_gap_after_compaction_without_a_regrow(env, writer, consumed):
    ghost_scenario(env, 200 + 2 * (WRITERS + ["scattered"]).index(writer) + consumed, "f32", "cosine", writer, consumed, EVERY_PATH)


def test_gap_after_compaction_l2(env):
    """a never-written slot is at distance sum q_i^2 under l2: 1 for -e0, which every written row is farther from"""
    ghost_scenario(env, 220, "f32", "l2", "upsert", False, ["scan"])


def test_gap_after_compaction_bf16(env):
    ghost_scenario(env, 221, "bf16", "cosine", "upsert_device", True, ["scan", "i8_tile"])


# ------------------------------------------------------------------------------------------------------------------------
# (d) seeded random walks
# ------------------------------------------------------------------------------------------------------------------------
LOW, HIGH = 6000, 14000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walk_of_writes_deletes_and_compactions(env, seed):
    """Ten operations drawn from: append, overwrite scattered rows, write past a gap, delete, compact, reserve.  After each, the
    exact scan and two filter paths (in rotation: each of the five is taken four times) against the model, every query compared.
    The batch of a step holds -e0, two rows written in the step and two rows deleted or vacated so far."""
    rng = np.random.default_rng(300 + seed)
    ix, model = make(env)
    raw = rows_like(rng, 8192)
    ix.upsert(np.arange(8192, dtype=np.int64), raw)
    model.upsert(np.arange(8192, dtype=np.int64), raw)
    always_filter(ix)
    gone = [raw[0], raw[1]]        # vectors of rows deleted or vacated so far (before the first delete: two stored rows, found at home)
    done = []

    def nonzero_rows(slots):
        rows = model.read_rows()[slots]
        return [r[:DIM].copy() for r in rows if r.any()]

    for step in range(10):
        while True:
            op = ["append", "overwrite", "gap", "delete", "compact", "reserve"][rng.integers(6)]
            count, live = model.count(), model._live_slots()
            written, keep = [], None
            if op == "append":
                m = int(rng.integers(50, 701))
                if count + m > HIGH:
                    continue
                vecs = rows_like(rng, m)
                keep = write(env, ix, model, WRITERS[rng.integers(3)], count, vecs)
                written = [vecs[0], vecs[-1]]
            elif op == "overwrite":
                slots = np.sort(rng.choice(live, int(rng.integers(1, 301)), replace=False)).astype(np.int64)
                vecs = rows_like(rng, slots.size)
                ix.upsert(slots, vecs)
                model.upsert(slots, vecs)
                written = [vecs[0], vecs[-1]]
            elif op == "gap":
                first, m = count + int(rng.integers(100, 601)), int(rng.integers(50, 301))
                if first + m > HIGH:
                    continue
                vecs = rows_like(rng, m)
                keep = write(env, ix, model, WRITERS[rng.integers(3)], first, vecs)
                written = [vecs[0], vecs[-1]]
            elif op == "delete":
                victims = rng.choice(live, max(1, int(live.size * rng.uniform(0.01, 0.2))), replace=False).astype(np.int64)
                gone = (nonzero_rows(victims[:8])[:2] + gone)[:6]
                ix.delete(victims)
                model.delete(victims)
            elif op == "compact":
                if live.size == count or live.size < LOW:
                    continue
                gone = (nonzero_rows(live[-8:])[-2:] + gone)[:6]   # the last live rows move down: their old slots are vacated
                assert ix.compact() == model.compact()
            else:
                ix.reserve(count + int(rng.integers(1000, 8000)))
            break
        done.append(op)
        assert ix.count() == model.count() and ix.live_count() == model.live_count(), done
        assert LOW <= model.count() <= HIGH, done
        q = query_batch(rng, written + gone[:2])
        names = ["scan", FILTERS[(2 * step) % 5], FILTERS[(2 * step + 1) % 5]]
        compare(ix, reference(model, q, names), q, names, f"seed {seed} after {done}")
        del keep
    assert np.array_equal(ix.read_rows(), model.read_rows()), done
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# shadow contents after partial rebuilds equal a build from scratch
# ------------------------------------------------------------------------------------------------------------------------
def test_shadows_after_partial_rebuilds_equal_a_build_from_scratch(env):
    """After each write step the long-lived index's approximate scores are compared bit for bit with the numpy integer reference
    (int8) and with a fresh index that received the model's rows in one upsert (both shadows), within 2e-5 with the
    rounded-operand fp64 reference (2-byte), and the two indexes' worst error norm and wide-block count are equal."""
    torch, Index = env
    from codd_query_engine_amd import native

    rng = np.random.default_rng(41)
    n = 8192
    raw = rng.standard_normal((n, DIM)).astype(np.float32)
    raw[:, 0] += 3.0
    ix, model = make(env)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    model.upsert(np.arange(n, dtype=np.int64), raw)
    q8 = rng.standard_normal((32, DIM)).astype(np.float32)
    q16 = rng.standard_normal((40, DIM)).astype(np.float32)
    shadow = "f16" if "shadow=f16" in native.load().codd_knn_version().decode() else "bf16"
    qb = o.widen(o.to_storage(o.normalize_rows(q16), shadow), shadow).astype(np.float64)

    def scores(index, q, shadow8):
        index.set_option("shadow8", shadow8)
        got = index.approx_scores(q).cpu().numpy()
        index.set_option("shadow8", 1)
        assert not got[q.shape[0]:].any()
        return got[: q.shape[0]]

    def same(got, want, what):
        differ = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=0))
        assert differ.size == 0 and not np.isnan(got).any(), (what, "rows", differ[:8].tolist(), differ.size, got[0, differ[:4]], want[0, differ[:4]])

    def check(what):
        rows = model.read_rows()
        assert model.live_count() == model.count() == ix.count(), what
        differ = np.flatnonzero((ix.read_rows() != rows).any(axis=1))
        assert differ.size == 0, (what, "stored rows differ from the model's", differ[:8].tolist(), differ.size)
        fresh = Index(DIM)
        fresh.upsert(np.arange(rows.shape[0], dtype=np.int64), rows[:, :DIM], normalize=False)
        assert np.array_equal(fresh.read_rows(), rows)
        mine, theirs = scores(ix, q8, 1), scores(fresh, q8, 1)
        same(mine, int8_scores(rows, o.normalize_rows(q8)), what + ": int8 shadow against the integer reference")
        same(mine, theirs, what + ": int8 shadow against a build from scratch")
        torch.cuda.synchronize()
        for key in ("shadow8_eps_r_micro", "shadow8_wide_blocks"):
            assert ix.stat(key) == fresh.stat(key), (what, key)
        mine, theirs = scores(ix, q16, 0), scores(fresh, q16, 0)
        same(mine, theirs, what + ": 2-byte shadow against a build from scratch")
        cb = o.widen(o.to_storage(rows, shadow), shadow).astype(np.float64)
        assert np.abs(mine - qb @ cb.T).max() < 2e-5, what
        fresh.close()

    def upsert(slots, vecs):
        slots = np.asarray(slots, dtype=np.int64)
        ix.upsert(slots, vecs)
        model.upsert(slots, vecs)

    def block_scale(row):
        return quantise_like_the_kernels(model.read_rows(), False)[1][row]

    check("built")
    spike = 4096 + 13                                               # in the middle of block 128
    assert block_scale(spike) < 0.003
    one_hot = np.zeros((1, DIM), dtype=np.float32)
    one_hot[0, 5] = 1.0
    upsert([spike], one_hot)
    assert block_scale(spike) == np.float32(1.0) / np.float32(127.0)
    check("one-hot row: the block's scale jumps to 1/127")
    upsert([spike], raw[spike : spike + 1])
    assert block_scale(spike) < 0.003
    check("ordinary row again: scale and error norm come down")
    more = rng.standard_normal((40, DIM)).astype(np.float32)
    more[:, 0] += 3.0
    upsert(np.arange(n, n + 13), more[:13])
    check("13 rows appended: block 256 partly filled")
    upsert(np.arange(n + 13, n + 38), more[13:38])
    check("25 more: block 256 quantised again")
    upsert([5, 8100], more[38:40])
    check("scattered upsert of slots 5 and 8,100")
    dead = np.arange(3000, 3500, dtype=np.int64)
    ix.delete(dead)
    model.delete(dead)
    assert ix.compact() == model.compact() == n + 38 - 500
    check("a middle range deleted and compacted")
    first = model.count() + 300
    upsert(np.arange(first, first + 50), rows_like(rng, 50))
    check("a gap write")
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------
# the per-block bound after a block's scale jumps
# ------------------------------------------------------------------------------------------------------------------------
def test_per_block_bound_follows_a_block_whose_scale_jumps(env):
    """Row v (flat, every element 1/sqrt(384)) shares a 32-row block with a row that becomes one-hot: the block's scale jumps to
    1/127, v quantises to 6 steps of it per element and its int8 score against itself drops to 0.926, with an error norm of
    0.074.  Ten near-copies of v in tile 0 (always sampled) put the threshold near 0.98: only the REBUILT block error norm
    lets v through the per-block bound — under the norm from before the jump (0.011) it would sit 0.05 below."""
    rng = np.random.default_rng(43)
    n, v, spike = 8192, 4096 + 7, 4096 + 16                       # block 128
    raw = rng.standard_normal((n, DIM)).astype(np.float32)
    raw[:, 0] += 3.0
    flat = np.full(DIM, 1.0 / np.sqrt(DIM), dtype=np.float32)
    raw[v] = flat
    planted = 20 + 13 * np.arange(10)
    for j, slot in enumerate(planted):
        raw[slot] = flat + np.float32(0.003 + 0.006 * j / 9) * rng.standard_normal(DIM).astype(np.float32)
    q = rng.standard_normal((140, DIM)).astype(np.float32)
    q[0] = flat
    qn = o.normalize_rows(q)
    ix, model = make(env)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    model.upsert(np.arange(n, dtype=np.int64), raw)
    always_filter(ix)

    rows = model.read_rows()
    assert row_error_norms(rows)[4096:4128].max() <= 0.02
    assert (rows[planted].astype(np.float64) @ qn[0].astype(np.float64) >= 0.98).all()
    compare(ix, reference(model, q, ["i8_tile"]), q, ["i8_tile"], "before the jump")      # builds the shadow

    one_hot = np.zeros((1, DIM), dtype=np.float32)
    one_hot[0, 5] = 1.0
    ix.upsert(np.array([spike], dtype=np.int64), one_hot)
    model.upsert(np.array([spike], dtype=np.int64), one_hot)
    rows = model.read_rows()
    assert int8_scores(rows, qn[:1])[0, v] <= 0.95 and row_error_norms(rows)[v] >= 0.06
    ref = reference(model, q, ["i8_tile"])
    assert ref[1][0, 0] == v and sorted(ref[1][0, 1:].tolist()) == sorted(planted[:9].tolist())
    dist, got = run_path(ix, "i8_tile", q)
    assert got[0, 0] == v and dist[0, 0] <= 2e-7, (got[0], dist[0])
    compare(ix, ref, q, ["i8_tile"], "after the jump")
    ix.close()
