"""Compile-time guard for the wide forms of the exact-score kernels (rows of more than 4 chunks per lane: f32 above 1,024
elements, 2-byte above 2,048).  The query lives in LDS and the row is walked in segments so that no instantiation needs more
registers than NITER 4 does; a spill would still compute the right scores, only with a scratch round trip in the row loop.
Same recipe as tests/test_kernel_resources.py: hipcc's own resource report, no GPU."""

import pytest

from tests._kernel_report import resource_rows


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


# kernel -> template arguments after the dtype (NITER = 0 is the wide form); the wide scan runs 1, 4 or 8 queries per pass over
# f32 rows and 1 or 4 over 2-byte rows
WIDE = {
    "finalize_kernel": [f"0, {sl}>" for sl in (1, 2)],
    "anchor_thr_kernel": [f"0, {sl}>" for sl in (1, 2)],
    "ivf_scan_kernel": [f"0, {sl}>" for sl in (1, 2)],
    "ivf_scan_shared_kernel": [f"0, {sl}>" for sl in (1, 2)],
}


def wide_names():
    names = [f"{kern}<{dt}, {tail}" for kern, tails in WIDE.items() for dt in (0, 1, 2) for tail in tails]
    return names + [f"scan_topk_wide_kernel<{dt}, {nb}, {sl}>" for dt in (0, 1, 2) for nb in ((1, 4, 8) if dt == 0 else (1, 4)) for sl in (1, 2)]


def test_every_wide_instantiation_is_built(rows):
    missing = [n for n in wide_names() if not any(name.endswith(n) for name in rows)]
    assert not missing, missing


@pytest.mark.parametrize("name", wide_names())
def test_wide_instantiation_neither_spills_nor_uses_scratch(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    r = hit[0]
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)


@pytest.mark.parametrize("name", [n for n in wide_names() if n.startswith("scan_topk_wide_kernel")])
def test_wide_scan_keeps_two_waves_per_simd(rows, name):
    r = next(r for key, r in rows.items() if key.endswith(name))
    assert r["occ"] >= 2, (name, r)
