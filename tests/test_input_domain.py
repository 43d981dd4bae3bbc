"""The input domain of the cosine, on the CPU: tiny, huge and non-finite vectors through the oracle, against tests/_cosine_reference.py
(fp64 from the RAW inputs; tolerance and comparison rule derived in its docstring).

The oracle restates the kernels' normalisation literally (canonical_norm in codd_knn.hip), so what fails here fails on the GPU the same
way; tests/test_gpu_input_domain.py then holds the kernels to the oracle bit for bit, and to the same fp64 reference."""

import importlib.util
import os

import numpy as np
import pytest

from oracle import knn_oracle as o
from tests import _cosine_reference as ref

WIDTHS = (64, 100, 768, 4096)
CONSTANTS = (4.47e-23, 3e-23, 2e-23, 1e-30, 1e-42, 1e18, 3e38)
EXPONENTS = (-140, -100, -75, -70, -64, 60, 63, 100)
DTYPES = ("f32", "bf16", "f16")


def fp64_norms(rows_f32):
    r = rows_f32.astype(np.float64)
    return np.sqrt((r * r).sum(axis=1))


def scaled_randn(rng, n, d, e):
    """randn * 2^e in fp32 (the product is rounded once: exact unless it lands among the subnormals)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(rng.standard_normal((n, d)), e).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the premise: this process computes with subnormals (a library linked with -ffast-math switches its loader to flush-to-zero;
# the HNSW comparator of bench.py used to be one, and the oracle and numpy then saw every subnormal input as zero)
# ------------------------------------------------------------------------------------------------------------------------
def test_loading_the_hnsw_comparator_leaves_subnormals_alone():
    from oracle import hnsw_cpu

    hnsw_cpu.lib()
    x = np.array([1e-42, -1e-45, 2.0**-127], dtype=np.float32)
    assert (x != 0).all() and (x * np.float32(1.0) == x).all() and (x.astype(np.float64) != 0).all()
    assert (np.ldexp(x, 100).astype(np.float64) == x.astype(np.float64) * 2.0**100).all()
    rows = o.normalize_rows(np.full((1, 64), 1e-42, dtype=np.float32))
    assert abs(fp64_norms(rows)[0] - 1.0) <= ref.delta(64)


# ------------------------------------------------------------------------------------------------------------------------
# stored norms
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("value", CONSTANTS)
def test_constant_vectors_are_stored_at_unit_norm(d, value):
    x = np.full((3, d), value, dtype=np.float32)
    x[1] = -x[1]
    x[2, ::2] = -x[2, ::2]
    assert np.isfinite(x).all() and (x != 0).all()
    rows = o.normalize_rows(x)
    dev = np.abs(fp64_norms(rows) - 1.0).max()
    print(f"d = {d}, every element {value:g}: |norm - 1| = {dev:.3e}, delta = {ref.delta(o.pad_dim(d)):.3e}")
    assert dev <= ref.delta(o.pad_dim(d))
    # a constant vector has one direction: 1 / sqrt(d) per element, with the signs of the input
    assert np.abs(rows[:, :d].astype(np.float64) - np.sign(x) / np.sqrt(d)).max() <= 2 * ref.delta(o.pad_dim(d)) / np.sqrt(d)


def scaled_case(d, e):
    return scaled_randn(np.random.default_rng(4100 + d + e), 16, d, e)


# "keep only the e for which randn * 2^e is finite and non-zero in fp32": decided once, from the seeded inputs themselves
SCALED = [(d, e) for d in WIDTHS for e in EXPONENTS if np.isfinite(scaled_case(d, e)).all() and (scaled_case(d, e) != 0).all()]


def test_only_the_exponent_fp32_cannot_hold_is_left_out():
    """at 2^-140 an element below 2^-150 rounds to zero (one in a thousand does); every other exponent of the list is tested at every width"""
    assert {(d, e) for d in WIDTHS for e in EXPONENTS if e != -140} <= set(SCALED)


@pytest.mark.parametrize("d,e", SCALED)
def test_scaled_normal_vectors_are_stored_at_unit_norm(d, e):
    x = scaled_case(d, e)
    rows = o.normalize_rows(x)
    dev = np.abs(fp64_norms(rows) - 1.0).max()
    print(f"d = {d}, randn * 2^{e}: |norm - 1| = {dev:.3e}, delta = {ref.delta(o.pad_dim(d)):.3e}")
    assert dev <= ref.delta(o.pad_dim(d))
    want = ref.unit64(x)
    assert (np.abs(rows.astype(np.float64) - want) <= 2 * ref.delta(o.pad_dim(d)) * np.abs(want)).all()


@pytest.mark.parametrize("d", (64, 100, 768))
def test_subnormal_elements_with_a_few_zeros_are_stored_at_unit_norm(d):
    """randn * 2^-140 holds subnormals that rounded to a few bits, and zeros: finite, non-zero VECTORS all the same"""
    rng = np.random.default_rng(4300 + d)
    x = scaled_randn(rng, 16, d, -140)
    assert (np.abs(x[x != 0]) < 2.0**-126).all() and (x != 0).any(axis=1).all()
    rows = o.normalize_rows(x)
    assert np.abs(fp64_norms(rows) - 1.0).max() <= ref.delta(o.pad_dim(d))
    one = np.zeros((1, d), dtype=np.float32)
    one[0, d // 2] = np.float32(1e-45)                                        # the smallest subnormal, alone
    assert np.array_equal(o.normalize_rows(one)[0, :d], (np.arange(d) == d // 2).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------
# scale invariance inside the normal range, bit for bit: the fix leaves today's expression alone
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (100, 768, 4096))
def test_power_of_two_scaling_changes_no_bit(d):
    rng = np.random.default_rng(4400 + d)
    raw = rng.standard_normal((200, d)).astype(np.float32)
    q = rng.standard_normal((4, d)).astype(np.float32)
    raw[np.abs(raw) < 2.0**-20] = 0.0
    q[np.abs(q) < 2.0**-20] = 0.0
    rows0, qn0 = o.normalize_rows(raw), o.normalize_rows(q)
    for e in (-40, -1, 1, 40):
        rows = o.normalize_rows(np.ldexp(raw, e))
        qn = o.normalize_rows(np.ldexp(q, e))
        assert np.array_equal(qn.view(np.uint32), qn0.view(np.uint32)), e
        for dtype in DTYPES:
            a, b = o.to_storage(rows, dtype), o.to_storage(rows0, dtype)
            assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), (e, dtype)
            assert np.array_equal(o.search_keys(a, dtype, qn, 10), o.search_keys(b, dtype, qn0, 10)), (e, dtype)


# ------------------------------------------------------------------------------------------------------------------------
# cosine end to end: corpora that mix unit-scale, tiny, huge and zero vectors
# ------------------------------------------------------------------------------------------------------------------------
ROW_SCALES = (0, -75, -100, -127, 63, 100, 0, -64, 60, 0)
N_MIXED, B_MIXED, K_MIXED = 48, 24, 5    # (five planted neighbours: at d = 100 ten bf16-decided scores above the background exceed |q| = 1)


def mixed_generator(seed, d, dtype):
    """48 rows and 24 queries at cycling scales (a few rows and queries zero); the queries are crafted against the stored rows so
    that the fp64 ranking of their five neighbours is decided whatever the storage type (tests/_cosine_reference.py)"""
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((N_MIXED, d)).astype(np.float32)
    for r in range(N_MIXED):
        raw[r] = np.ldexp(raw[r], ROW_SCALES[r % len(ROW_SCALES)])
    raw[7] = 0.0
    raw[N_MIXED - 1] = 0.0
    raw[11] = np.float32(4.47e-23)
    assert np.isfinite(raw).all()
    live = np.flatnonzero(~ref.is_zero_vector(raw))
    t = ref.tol(dtype, o.pad_dim(d))
    picks = np.stack([rng.choice(live, size=K_MIXED, replace=False) for _ in range(B_MIXED)])
    # 48 rows: the background reaches 3 / sqrt(d) at the most
    q = ref.crafted_queries(raw, dtype, picks, t, floor=3.0 / np.sqrt(d))
    for b in range(B_MIXED):
        q[b] = np.ldexp(q[b], (0, -80, 90, -100, 40, 0)[b % 6])
    q[5] = 0.0
    assert np.isfinite(q).all()
    return raw, q, picks


MIXED = [(d, dtype) for d in (100, 768) for dtype in DTYPES]


@pytest.mark.parametrize("d,dtype", MIXED)
def test_the_reference_alone_decides_nine_positions_in_ten(d, dtype):
    """the generator, judged without any code under test: the fp64 ranking is decided at >= 90 % of the positions, and the
    decided ranking is the one the generator planted"""
    raw, q, picks = mixed_generator(4500 + d, d, dtype)
    t = ref.tol(dtype, o.pad_dim(d))
    live = ~ref.is_zero_vector(q)
    ids, dec = ref.decided(ref.scores64(q, raw, dtype)[live], K_MIXED, t)
    share = 1.0 - dec.mean()
    print(f"mixed corpus d = {d} {dtype}: the reference leaves out {share:.1%}, cap {ref.CAP:.0%}")
    assert share <= ref.CAP
    assert np.array_equal(ids[dec], picks[live][dec])


@pytest.mark.parametrize("d,dtype", MIXED)
def test_search_over_mixed_scales_agrees_with_fp64_cosine(d, dtype):
    raw, q, _ = mixed_generator(4500 + d, d, dtype)
    rows = o.to_storage(o.normalize_rows(raw), dtype)
    dist, ids = o.search(rows, dtype, o.normalize_rows(q), K_MIXED)
    ref.check(dist, ids, q, ref.scores64(q, raw, dtype), ref.tol(dtype, o.pad_dim(d)), what=f"mixed d = {d} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_scaled_copy_of_a_row_finds_it_at_distance_zero(dtype):
    d = 768
    rng = np.random.default_rng(4600)
    raw = rng.standard_normal((300, d)).astype(np.float32)
    raw[40] = np.ldexp(raw[40], -100)
    raw[41] = np.ldexp(raw[41], 100)
    q = np.stack([np.ldexp(raw[17], -90), np.ldexp(raw[17], 80), np.ldexp(raw[40], 190), np.ldexp(raw[41], -190), np.ldexp(raw[40], -10)])
    assert np.isfinite(q).all() and (q != 0).any(axis=1).all()
    rows = o.to_storage(o.normalize_rows(raw), dtype)
    dist, ids = o.search(rows, dtype, o.normalize_rows(q), 10)
    t = ref.tol(dtype, o.pad_dim(d))
    assert ids[:, 0].tolist() == [17, 17, 40, 41, 40]
    assert np.abs(dist[:, 0]).max() <= t, (dist[:, 0], t)
    assert (dist >= -t).all(), "a similarity above 1"
    ref.check(dist[:, :1], ids[:, :1], q, ref.scores64(q, raw, dtype), t, what=f"scaled copies {dtype}")


# ------------------------------------------------------------------------------------------------------------------------
# non-finite values
# ------------------------------------------------------------------------------------------------------------------------
BAD = (np.nan, np.inf, -np.inf)


@pytest.mark.parametrize("d", (100, 768))
@pytest.mark.parametrize("scale", (0, -100, 100))
def test_a_non_finite_element_makes_the_zero_vector(d, scale):
    rng = np.random.default_rng(4700 + d)
    x = scaled_randn(rng, 3 * 4, d, scale)
    where = (0, d // 2, d - 1, 5)
    for i, bad in enumerate(BAD):
        for j, pos in enumerate(where):
            x[i * 4 + j, pos] = bad
    x[3, 0] = np.inf                                                           # NaN and inf in one row
    rows = o.normalize_rows(x)
    assert rows.shape == (12, o.pad_dim(d)) and not rows.any(), "a non-finite element left something behind"
    assert not (rows.view(np.uint32) & 0x80000000).any(), "negative zeros"


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows_and_queries_score_zero_at_distance_one(dtype):
    d, n, k = 100, 60, 12
    rng = np.random.default_rng(4800)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    bad_rows = {3: np.nan, 20: np.inf, 41: -np.inf}
    for r, bad in bad_rows.items():
        raw[r, r % d] = bad
    q = rng.standard_normal((7, d)).astype(np.float32)
    q[0, 0] = np.nan
    q[3, d - 1] = np.inf
    q[6, 50] = -np.inf
    rows = o.to_storage(o.normalize_rows(raw), dtype)
    for r in bad_rows:
        assert not rows[r].any()
    dist, ids = o.search(rows, dtype, o.normalize_rows(q), k)
    assert np.isfinite(dist[ids >= 0]).all() and (ids >= 0).all()
    for b in (0, 3, 6):                                                        # a zero query: rows 0 .. k - 1 at distance exactly 1
        assert ids[b].tolist() == list(range(k)) and (dist[b] == 1.0).all()
    # every row against the finite queries: a non-finite row sits at distance exactly 1
    dist, ids = o.search(rows, dtype, o.normalize_rows(q[[1, 2, 4, 5]]), n)
    assert np.isfinite(dist).all() and (np.sort(ids, axis=1) == np.arange(n)).all()
    for r in bad_rows:
        assert (dist[ids == r] == 1.0).all()
    t = ref.tol(dtype, o.pad_dim(d))
    S = ref.scores64(q, raw, dtype)
    assert (S[[0, 3, 6]] == 0).all() and (S[:, list(bad_rows)] == 0).all()
    got = 1.0 - dist.astype(np.float64)
    assert np.abs(got - np.take_along_axis(S[[1, 2, 4, 5]], ids, axis=1)).max() <= t


# ------------------------------------------------------------------------------------------------------------------------
# the committed golden vectors: the generator reproduces them bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def test_the_generator_reproduces_the_committed_golden_vectors(golden_dir, tmp_path, monkeypatch):
    path = os.path.join(os.path.dirname(golden_dir), os.pardir, "oracle", "gen_knn_golden.py")
    spec = importlib.util.spec_from_file_location("gen_knn_golden_under_test", os.path.normpath(path))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "knn_golden.npz"
    monkeypatch.setattr(gen, "OUT", str(out))
    gen.main()
    new, old = np.load(out), np.load(os.path.join(golden_dir, "knn_golden.npz"))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        a, b = new[key], old[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
