"""Compile-time guard for the tombstone argument, after tests/test_scoped_kernel_resources.py: hipcc's own resource
report, no GPU.  The kernels that take the `dead` bitmap must not have started to spill or to use scratch because of it, the forms
on the headline path — finalize_fb_kernel behind i8_tile_kernel<FILTER, 3> — keep the occupancy they had, the MFMA filters (which
take no bitmap: dead rows may produce hits, finalize drops them) are what they were, and the new kernels are tiny.

BEFORE_OCC: the occupancy of the same instantiations in the build before tombstones existed, taken from that build's report."""

import pytest

from tests._kernel_report import resource_rows


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


def find(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    return hit[0]


# every instantiation the dispatch can reach of the kernels that now take the bitmap (finalize_fb_kernel<2-byte, 4> is built but
# never launched: filter_pass sends those rows to finalize_kernel + the list-driven scan, as before)
FINALIZE_FB = [f"finalize_fb_kernel<{dt}, {ni}>" for dt in (0, 1, 2) for ni in (1, 2, 3, 4) if not (dt != 0 and ni == 4)]
MASKED = (FINALIZE_FB
          + [f"finalize_kernel<{dt}, {ni}, {sl}>" for dt in (0, 1, 2) for ni in (1, 2, 3, 4, 0) for sl in (1, 2)]
          + [f"anchor_thr_kernel<{dt}, {ni}, {sl}>" for dt in (0, 1, 2) for ni in (1, 2, 3, 4, 0) for sl in (1, 2)]
          + [f"scan_topk_kernel<{dt}, {nb}, {ni}, {sl}>" for dt in (0, 1, 2) for nb in (1, 4, 8) for ni in (1, 2, 3, 4) for sl in (1, 2)]
          + [f"scan_topk_wide_kernel<{dt}, {nb}, {sl}>" for dt in (0, 1, 2) for nb in (1, 4, 8) for sl in (1, 2) if not (dt != 0 and nb == 8)]
          + [f"ivf_scan_kernel<{dt}, {ni}, {sl}>" for dt in (0, 1, 2) for ni in (1, 2, 3, 4, 0) for sl in (1, 2)]
          + [f"ivf_scan_shared_kernel<{dt}, {ni}, {sl}>" for dt in (0, 1, 2) for ni in (1, 2, 3, 4, 0) for sl in (1, 2) if not (dt != 0 and ni == 4)]
          + [f"small_batch_kernel<{dt}, {ni}, {ns}>" for dt, ni, ns in ((0, 2, 3), (0, 2, 4), (0, 3, 6), (0, 4, 8), (1, 1, 3), (1, 1, 4), (1, 2, 6), (1, 2, 8))])

# occupancy (waves per SIMD) of every one of them in the build before tombstones existed, from that build's own report
BEFORE_OCC = {
    "finalize_fb_kernel<0, 1>": 4, "finalize_fb_kernel<0, 2>": 3, "finalize_fb_kernel<0, 3>": 3, "finalize_fb_kernel<0, 4>": 2, "finalize_fb_kernel<1, 1>": 3,
    "finalize_fb_kernel<1, 2>": 2, "finalize_fb_kernel<1, 3>": 2, "finalize_fb_kernel<2, 1>": 4, "finalize_fb_kernel<2, 2>": 2, "finalize_fb_kernel<2, 3>": 2,
    "finalize_kernel<0, 1, 1>": 8, "finalize_kernel<0, 1, 2>": 7, "finalize_kernel<0, 2, 1>": 5, "finalize_kernel<0, 2, 2>": 5, "finalize_kernel<0, 3, 1>": 4,
    "finalize_kernel<0, 3, 2>": 4, "finalize_kernel<0, 4, 1>": 4, "finalize_kernel<0, 4, 2>": 3, "finalize_kernel<0, 0, 1>": 2, "finalize_kernel<0, 0, 2>": 2,
    "finalize_kernel<1, 1, 1>": 5, "finalize_kernel<1, 1, 2>": 5, "finalize_kernel<1, 2, 1>": 4, "finalize_kernel<1, 2, 2>": 3, "finalize_kernel<1, 3, 1>": 3,
    "finalize_kernel<1, 3, 2>": 2, "finalize_kernel<1, 4, 1>": 2, "finalize_kernel<1, 4, 2>": 2, "finalize_kernel<1, 0, 1>": 2, "finalize_kernel<1, 0, 2>": 2,
    "finalize_kernel<2, 1, 1>": 7, "finalize_kernel<2, 1, 2>": 6, "finalize_kernel<2, 2, 1>": 5, "finalize_kernel<2, 2, 2>": 4, "finalize_kernel<2, 3, 1>": 4,
    "finalize_kernel<2, 3, 2>": 4, "finalize_kernel<2, 4, 1>": 3, "finalize_kernel<2, 4, 2>": 3, "finalize_kernel<2, 0, 1>": 3, "finalize_kernel<2, 0, 2>": 2,
    "anchor_thr_kernel<0, 1, 1>": 8, "anchor_thr_kernel<0, 1, 2>": 8, "anchor_thr_kernel<0, 2, 1>": 8, "anchor_thr_kernel<0, 2, 2>": 8, "anchor_thr_kernel<0, 3, 1>": 5,
    "anchor_thr_kernel<0, 3, 2>": 5, "anchor_thr_kernel<0, 4, 1>": 4, "anchor_thr_kernel<0, 4, 2>": 4, "anchor_thr_kernel<0, 0, 1>": 4, "anchor_thr_kernel<0, 0, 2>": 4,
    "anchor_thr_kernel<1, 1, 1>": 8, "anchor_thr_kernel<1, 1, 2>": 8, "anchor_thr_kernel<1, 2, 1>": 4, "anchor_thr_kernel<1, 2, 2>": 4, "anchor_thr_kernel<1, 3, 1>": 3,
    "anchor_thr_kernel<1, 3, 2>": 3, "anchor_thr_kernel<1, 4, 1>": 2, "anchor_thr_kernel<1, 4, 2>": 2, "anchor_thr_kernel<1, 0, 1>": 2, "anchor_thr_kernel<1, 0, 2>": 2,
    "anchor_thr_kernel<2, 1, 1>": 8, "anchor_thr_kernel<2, 1, 2>": 8, "anchor_thr_kernel<2, 2, 1>": 7, "anchor_thr_kernel<2, 2, 2>": 7, "anchor_thr_kernel<2, 3, 1>": 5,
    "anchor_thr_kernel<2, 3, 2>": 5, "anchor_thr_kernel<2, 4, 1>": 4, "anchor_thr_kernel<2, 4, 2>": 4, "anchor_thr_kernel<2, 0, 1>": 3, "anchor_thr_kernel<2, 0, 2>": 3,
    "scan_topk_kernel<0, 1, 1, 1>": 7, "scan_topk_kernel<0, 1, 1, 2>": 7, "scan_topk_kernel<0, 1, 2, 1>": 5, "scan_topk_kernel<0, 1, 2, 2>": 5, "scan_topk_kernel<0, 1, 3, 1>": 4,
    "scan_topk_kernel<0, 1, 3, 2>": 4, "scan_topk_kernel<0, 1, 4, 1>": 4, "scan_topk_kernel<0, 1, 4, 2>": 3, "scan_topk_kernel<0, 4, 1, 1>": 5, "scan_topk_kernel<0, 4, 1, 2>": 4,
    "scan_topk_kernel<0, 4, 2, 1>": 4, "scan_topk_kernel<0, 4, 2, 2>": 3, "scan_topk_kernel<0, 4, 3, 1>": 3, "scan_topk_kernel<0, 4, 3, 2>": 3, "scan_topk_kernel<0, 4, 4, 1>": 2,
    "scan_topk_kernel<0, 4, 4, 2>": 2, "scan_topk_kernel<0, 8, 1, 1>": 4, "scan_topk_kernel<0, 8, 1, 2>": 3, "scan_topk_kernel<0, 8, 2, 1>": 2, "scan_topk_kernel<0, 8, 2, 2>": 2,
    "scan_topk_kernel<0, 8, 3, 1>": 2, "scan_topk_kernel<0, 8, 3, 2>": 2, "scan_topk_kernel<0, 8, 4, 1>": 1, "scan_topk_kernel<0, 8, 4, 2>": 1, "scan_topk_kernel<1, 1, 1, 1>": 5,
    "scan_topk_kernel<1, 1, 1, 2>": 5, "scan_topk_kernel<1, 1, 2, 1>": 4, "scan_topk_kernel<1, 1, 2, 2>": 4, "scan_topk_kernel<1, 1, 3, 1>": 3, "scan_topk_kernel<1, 1, 3, 2>": 3,
    "scan_topk_kernel<1, 1, 4, 1>": 2, "scan_topk_kernel<1, 1, 4, 2>": 2, "scan_topk_kernel<1, 4, 1, 1>": 4, "scan_topk_kernel<1, 4, 1, 2>": 3, "scan_topk_kernel<1, 4, 2, 1>": 2,
    "scan_topk_kernel<1, 4, 2, 2>": 2, "scan_topk_kernel<1, 4, 3, 1>": 2, "scan_topk_kernel<1, 4, 3, 2>": 1, "scan_topk_kernel<1, 4, 4, 1>": 1, "scan_topk_kernel<1, 4, 4, 2>": 1,
    "scan_topk_kernel<1, 8, 1, 1>": 2, "scan_topk_kernel<1, 8, 1, 2>": 2, "scan_topk_kernel<1, 8, 2, 1>": 1, "scan_topk_kernel<1, 8, 2, 2>": 1, "scan_topk_kernel<1, 8, 3, 1>": 1,
    "scan_topk_kernel<1, 8, 3, 2>": 1, "scan_topk_kernel<1, 8, 4, 1>": 1, "scan_topk_kernel<1, 8, 4, 2>": 1, "scan_topk_kernel<2, 1, 1, 1>": 6, "scan_topk_kernel<2, 1, 1, 2>": 6,
    "scan_topk_kernel<2, 1, 2, 1>": 5, "scan_topk_kernel<2, 1, 2, 2>": 5, "scan_topk_kernel<2, 1, 3, 1>": 4, "scan_topk_kernel<2, 1, 3, 2>": 4, "scan_topk_kernel<2, 1, 4, 1>": 3,
    "scan_topk_kernel<2, 1, 4, 2>": 3, "scan_topk_kernel<2, 4, 1, 1>": 4, "scan_topk_kernel<2, 4, 1, 2>": 4, "scan_topk_kernel<2, 4, 2, 1>": 2, "scan_topk_kernel<2, 4, 2, 2>": 2,
    "scan_topk_kernel<2, 4, 3, 1>": 2, "scan_topk_kernel<2, 4, 3, 2>": 2, "scan_topk_kernel<2, 4, 4, 1>": 1, "scan_topk_kernel<2, 4, 4, 2>": 1, "scan_topk_kernel<2, 8, 1, 1>": 3,
    "scan_topk_kernel<2, 8, 1, 2>": 2, "scan_topk_kernel<2, 8, 2, 1>": 1, "scan_topk_kernel<2, 8, 2, 2>": 1, "scan_topk_kernel<2, 8, 3, 1>": 1, "scan_topk_kernel<2, 8, 3, 2>": 1,
    "scan_topk_kernel<2, 8, 4, 1>": 1, "scan_topk_kernel<2, 8, 4, 2>": 1, "scan_topk_wide_kernel<0, 1, 1>": 3, "scan_topk_wide_kernel<0, 1, 2>": 3, "scan_topk_wide_kernel<0, 4, 1>": 2,
    "scan_topk_wide_kernel<0, 4, 2>": 2, "scan_topk_wide_kernel<0, 8, 1>": 2, "scan_topk_wide_kernel<0, 8, 2>": 2, "scan_topk_wide_kernel<1, 1, 1>": 2, "scan_topk_wide_kernel<1, 1, 2>": 2,
    "scan_topk_wide_kernel<1, 4, 1>": 2, "scan_topk_wide_kernel<1, 4, 2>": 2, "scan_topk_wide_kernel<2, 1, 1>": 2, "scan_topk_wide_kernel<2, 1, 2>": 2, "scan_topk_wide_kernel<2, 4, 1>": 2,
    "scan_topk_wide_kernel<2, 4, 2>": 2, "ivf_scan_kernel<0, 1, 1>": 8, "ivf_scan_kernel<0, 1, 2>": 8, "ivf_scan_kernel<0, 2, 1>": 7, "ivf_scan_kernel<0, 2, 2>": 6,
    "ivf_scan_kernel<0, 3, 1>": 5, "ivf_scan_kernel<0, 3, 2>": 4, "ivf_scan_kernel<0, 4, 1>": 4, "ivf_scan_kernel<0, 4, 2>": 4, "ivf_scan_kernel<0, 0, 1>": 4,
    "ivf_scan_kernel<0, 0, 2>": 4, "ivf_scan_kernel<1, 1, 1>": 7, "ivf_scan_kernel<1, 1, 2>": 6, "ivf_scan_kernel<1, 2, 1>": 4, "ivf_scan_kernel<1, 2, 2>": 4,
    "ivf_scan_kernel<1, 3, 1>": 3, "ivf_scan_kernel<1, 3, 2>": 3, "ivf_scan_kernel<1, 4, 1>": 2, "ivf_scan_kernel<1, 4, 2>": 2, "ivf_scan_kernel<1, 0, 1>": 2,
    "ivf_scan_kernel<1, 0, 2>": 2, "ivf_scan_kernel<2, 1, 1>": 8, "ivf_scan_kernel<2, 1, 2>": 8, "ivf_scan_kernel<2, 2, 1>": 6, "ivf_scan_kernel<2, 2, 2>": 5,
    "ivf_scan_kernel<2, 3, 1>": 4, "ivf_scan_kernel<2, 3, 2>": 4, "ivf_scan_kernel<2, 4, 1>": 4, "ivf_scan_kernel<2, 4, 2>": 3, "ivf_scan_kernel<2, 0, 1>": 3,
    "ivf_scan_kernel<2, 0, 2>": 3, "ivf_scan_shared_kernel<0, 1, 1>": 5, "ivf_scan_shared_kernel<0, 1, 2>": 4, "ivf_scan_shared_kernel<0, 2, 1>": 3, "ivf_scan_shared_kernel<0, 2, 2>": 3,
    "ivf_scan_shared_kernel<0, 3, 1>": 2, "ivf_scan_shared_kernel<0, 3, 2>": 2, "ivf_scan_shared_kernel<0, 4, 1>": 2, "ivf_scan_shared_kernel<0, 4, 2>": 2, "ivf_scan_shared_kernel<0, 0, 1>": 2,
    "ivf_scan_shared_kernel<0, 0, 2>": 2, "ivf_scan_shared_kernel<1, 1, 1>": 4, "ivf_scan_shared_kernel<1, 1, 2>": 4, "ivf_scan_shared_kernel<1, 2, 1>": 3, "ivf_scan_shared_kernel<1, 2, 2>": 2,
    "ivf_scan_shared_kernel<1, 3, 1>": 2, "ivf_scan_shared_kernel<1, 3, 2>": 2, "ivf_scan_shared_kernel<1, 0, 1>": 2, "ivf_scan_shared_kernel<1, 0, 2>": 2, "ivf_scan_shared_kernel<2, 1, 1>": 4,
    "ivf_scan_shared_kernel<2, 1, 2>": 4, "ivf_scan_shared_kernel<2, 2, 1>": 3, "ivf_scan_shared_kernel<2, 2, 2>": 2, "ivf_scan_shared_kernel<2, 3, 1>": 2, "ivf_scan_shared_kernel<2, 3, 2>": 2,
    "ivf_scan_shared_kernel<2, 0, 1>": 2, "ivf_scan_shared_kernel<2, 0, 2>": 2, "small_batch_kernel<0, 2, 3>": 4, "small_batch_kernel<0, 2, 4>": 4, "small_batch_kernel<0, 3, 6>": 2,
    "small_batch_kernel<0, 4, 8>": 2, "small_batch_kernel<1, 1, 3>": 4, "small_batch_kernel<1, 1, 4>": 4, "small_batch_kernel<1, 2, 6>": 2, "small_batch_kernel<1, 2, 8>": 2,
}
HEADLINE_TILE = (254, 2, 0, 0)   # i8_tile_kernel<FILTER, 3, 16 query blocks>: vgpr, occupancy, spill, scratch


def test_no_masked_instantiation_spills_or_uses_scratch(rows):
    bad = [(name, find(rows, name)) for name in MASKED]
    bad = [(name, r) for name, r in bad if r["spill"] or r["scratch"] or r["sspill"]]
    assert not bad, bad


def test_masked_forms_keep_their_occupancy(rows):
    assert set(BEFORE_OCC) == set(MASKED)
    worse = [(name, find(rows, name)["occ"], BEFORE_OCC[name]) for name in MASKED if find(rows, name)["occ"] < BEFORE_OCC[name]]
    assert not worse, worse


def test_the_headline_pair_is_untouched_or_no_worse(rows):
    tile = find(rows, "i8_tile_kernel<0, 3, 16, false, false>")   # (MODE_FILTER = 0)
    assert (tile["vgpr"], tile["occ"], tile["spill"], tile["scratch"]) == HEADLINE_TILE, tile
    fin = find(rows, "finalize_fb_kernel<0, 3>")   # f32 rows of 768 elements: 3 chunks per lane
    assert fin["occ"] >= BEFORE_OCC["finalize_fb_kernel<0, 3>"] == 3 and fin["spill"] == 0 and fin["scratch"] == 0, fin


def test_the_new_kernels_are_built_and_tiny(rows):
    for kern in ("dead_set_kernel", "live_prefix_kernel", "compact_gather_kernel"):
        r = find(rows, kern)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sspill"] == 0 and r["vgpr"] <= 32, (kern, r)
