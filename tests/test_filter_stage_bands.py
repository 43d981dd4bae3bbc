"""The cases of tests/test_gpu_filter_stages.py, without a device: the statements about a program's cut exempt the rows of an
ambiguity band (the per-block int8 programs: the fp32 roundings of the kernel's threshold expression plus three accumulator levels;
the 2-byte programs: the accumulation order, either side of the threshold).  A case says something only if that band is next to
empty: at most 1 % of the case's candidates and at most 8 rows of one query, by the REFERENCE alone — its own sample keys, anchors
and thresholds (tests/_filter_stage_reference.py) over the case's data, 256 compute units assumed for the sampled tiles of the large
cases.  For the int8 GEMM programs, whose cut is exact, the two ways of writing it are shown to name the same rows on this data:
fp32(acc s_row) >= fp32(thr / s_q), the kernel's, and s~ = fp32(fp32(acc s_row) s_q) >= thr."""

import numpy as np
import pytest

from tests import _filter_stage_reference as fs

BANDED = [c for c in fs.CASES if c.per_block or not c.el]
EXACT_GEMM = [c for c in fs.CASES if c.family == "GEMM" and c.el and not c.sqd and not c.multi]


def reference_pass(case):
    raw, q = fs.make_data(case)
    p = fs.Pass(case, fs.stored_rows(case.space, raw, case.dtype), q)
    ntiles = (p.n + fs.TILE - 1) // fs.TILE
    ts, stride = fs.sample_geometry(ntiles, fs.K, bool(case.el), case.nbq, 256)
    if case.el:
        qmeta, bmeta = fs.model_meta(p, raw, q)
    else:
        qmeta, bmeta = None, None
    L, thr, thr0 = p.anchors(fs.reference_keys(p, ts, stride), fs.K, fs.eps16_of(case.dtype, p.dpad), qmeta)
    return p, thr, thr0, qmeta, bmeta


@pytest.mark.parametrize("case", BANDED, ids=lambda c: c.id)
def test_ambiguity_band_is_next_to_empty(case):
    p, thr, thr0, qmeta, bmeta = reference_pass(case)
    assert np.isfinite(thr[: p.B]).all()
    cand, exempt, worst = fs.band_population(p, thr, thr0, qmeta, bmeta)
    print(case.id, "candidates", cand, "exempt", exempt, "most of one query", worst)
    assert cand >= 10 * p.B
    assert fs.band_is_valid(cand, exempt, worst), (cand, exempt, worst)


@pytest.mark.parametrize("case", EXACT_GEMM, ids=lambda c: c.id)
def test_both_forms_of_the_exact_cut_name_the_same_rows(case):
    p, thr, thr0, qmeta, bmeta = reference_pass(case)
    total = 0
    for q in range(p.B):
        must, _, _ = p.cut(q, thr, thr0, qmeta, bmeta)
        assert np.array_equal(must, p.score[q] >= thr[q]), q
        total += int(must.sum())
    assert total >= 10 * p.B


def test_every_program_of_the_issue_has_a_case():
    have = {(c.family, c.nbq, c.ts, c.res, c.el, c.sqd, c.space) for c in fs.CASES if not c.multi}
    want = [("GEMM", nbq, 0, 0, 0, 0, "cosine") for nbq in (1, 2, 4, 8)]
    want += [("GEMM", 1, 0, 0, 1, 0, "cosine"), ("GEMM", 2, 0, 0, 1, 0, "cosine"), ("GEMM", 4, 0, 2, 1, 0, "cosine")]
    want += [("GEMM", nbq, 0, 1, 1, 0, "cosine") for nbq in (1, 2, 4, 8)]
    want += [("TILE", nbq, ts, 0, 1, 0, "cosine") for ts in (0, 1, 2, 3) for nbq in (4, 8)]
    want += [("TILE", nbq, ts, 1, 1, 0, "cosine") for ts in (0, 1) for nbq in (4, 8)]
    want += [("GEMM", 4, 0, 0, 1, 0, "cosine"), ("GEMM", 8, 0, 0, 1, 0, "cosine")]
    want += [("GEMM", nbq, 0, 0, 1, 0, "ip") for nbq in (2, 4, 8)] + [("GEMM", 8, 0, 1, 1, 0, "ip"), ("GEMM", 4, 0, 2, 1, 0, "ip")]
    want += [("TILE_F16", 8, ts, 0, 0, 0, "cosine") for ts in (2, 3, 4)]
    want += [("GEMM", nbq, 0, 0, 1, 1, "l2") for nbq in (1, 2, 4, 8)]
    assert not [w for w in want if w not in have]
    assert len({(c.res, c.nbq) for c in fs.CASES if c.space == "ip"}) >= 2
    assert {"bf16", "f16"} <= {c.dtype for c in fs.CASES if c.family in ("TILE", "GEMM")}
    assert [c for c in fs.CASES if c.multi and (c.family, c.nbq, c.res) == ("TILE", 4, 1)], "parity lists over several tiles, 8 query blocks"
    multi = {(c.family, c.ts, c.res, c.el) for c in fs.CASES if c.multi}
    assert {("TILE", 0, 0, 1), ("TILE", 1, 0, 1), ("TILE", 2, 0, 1), ("TILE", 3, 0, 1), ("TILE", 1, 1, 1), ("TILE_F16", 3, 0, 0),
            ("TILE_F16", 4, 0, 0), ("GEMM", 0, 0, 1), ("GEMM", 0, 0, 0)} <= multi
