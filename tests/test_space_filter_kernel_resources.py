"""Compile-time guard for the kernels of the int8 filter leg of an ip or l2 index: every new kernel the routing can
reach — the squared-distance filter in its three modes, the threshold, finalize and listed-scan kernels for rows of 1 .. 4 chunks
per lane and one or two list slots, the row norms, the raw query preparation, the slack read-out — must be built and may neither
spill nor use scratch.  OCC is the occupancy of each in this build (waves per SIMD): a change is a change of the code or of the
compiler and is made on purpose.  The names keep clear of the guards of earlier commits: none contains "_l2<" or
"raw_rows_kernel<" (tests/test_spaces_kernel_resources.py counts those), none ends in or is the tail of a parent kernel's name.
That every parent kernel keeps its resource line is tests/test_spaces_kernel_resources.py's own check.  hipcc's resource report,
shared with the other guards; no GPU."""

import os

import pytest

from tests._kernel_report import resource_rows

FORMS = [(dt, niter, sl) for dt in (0, 1, 2) for niter in (1, 2, 3, 4) for sl in (1, 2)]
FILTER = [f"sqd_filter_kernel<{mode}, {nbq}>" for mode in (0, 1) for nbq in (1, 2, 4, 8)] + ["sqd_filter_kernel<2, 1>"]
ROWS = [f"{stem}<{dt}, {niter}, {sl}>" for stem in ("sqd_thr_kernel", "sqd_fin_kernel", "sqd_listed_scan_kernel") for dt, niter, sl in FORMS]
SMALL = ["row_sqnorm_kernel<0>", "row_sqnorm_kernel<1>", "row_sqnorm_kernel<2>", "prep_queries8_raw_kernel", "filter_slack_kernel"]
REACHED = FILTER + ROWS + SMALL

OCC = {
    "filter_slack_kernel": 8, "prep_queries8_raw_kernel": 8, "row_sqnorm_kernel<0>": 8, "row_sqnorm_kernel<1>": 8, "row_sqnorm_kernel<2>": 8,
    "sqd_filter_kernel<0, 1>": 4, "sqd_filter_kernel<0, 2>": 3, "sqd_filter_kernel<0, 4>": 3, "sqd_filter_kernel<0, 8>": 2, "sqd_filter_kernel<1, 1>": 4,
    "sqd_filter_kernel<1, 2>": 3, "sqd_filter_kernel<1, 4>": 3, "sqd_filter_kernel<1, 8>": 2, "sqd_filter_kernel<2, 1>": 4, "sqd_fin_kernel<0, 1, 1>": 8,
    "sqd_fin_kernel<0, 1, 2>": 7, "sqd_fin_kernel<0, 2, 1>": 5, "sqd_fin_kernel<0, 2, 2>": 5, "sqd_fin_kernel<0, 3, 1>": 4, "sqd_fin_kernel<0, 3, 2>": 4,
    "sqd_fin_kernel<0, 4, 1>": 4, "sqd_fin_kernel<0, 4, 2>": 3, "sqd_fin_kernel<1, 1, 1>": 7, "sqd_fin_kernel<1, 1, 2>": 6, "sqd_fin_kernel<1, 2, 1>": 5,
    "sqd_fin_kernel<1, 2, 2>": 4, "sqd_fin_kernel<1, 3, 1>": 4, "sqd_fin_kernel<1, 3, 2>": 4, "sqd_fin_kernel<1, 4, 1>": 3, "sqd_fin_kernel<1, 4, 2>": 3,
    "sqd_fin_kernel<2, 1, 1>": 7, "sqd_fin_kernel<2, 1, 2>": 6, "sqd_fin_kernel<2, 2, 1>": 5, "sqd_fin_kernel<2, 2, 2>": 4, "sqd_fin_kernel<2, 3, 1>": 4,
    "sqd_fin_kernel<2, 3, 2>": 4, "sqd_fin_kernel<2, 4, 1>": 3, "sqd_fin_kernel<2, 4, 2>": 3, "sqd_listed_scan_kernel<0, 1, 1>": 5, "sqd_listed_scan_kernel<0, 1, 2>": 4,
    "sqd_listed_scan_kernel<0, 2, 1>": 4, "sqd_listed_scan_kernel<0, 2, 2>": 3, "sqd_listed_scan_kernel<0, 3, 1>": 3, "sqd_listed_scan_kernel<0, 3, 2>": 3, "sqd_listed_scan_kernel<0, 4, 1>": 2,
    "sqd_listed_scan_kernel<0, 4, 2>": 2, "sqd_listed_scan_kernel<1, 1, 1>": 4, "sqd_listed_scan_kernel<1, 1, 2>": 3, "sqd_listed_scan_kernel<1, 2, 1>": 2, "sqd_listed_scan_kernel<1, 2, 2>": 2,
    "sqd_listed_scan_kernel<1, 3, 1>": 2, "sqd_listed_scan_kernel<1, 3, 2>": 1, "sqd_listed_scan_kernel<1, 4, 1>": 1, "sqd_listed_scan_kernel<1, 4, 2>": 1, "sqd_listed_scan_kernel<2, 1, 1>": 4,
    "sqd_listed_scan_kernel<2, 1, 2>": 3, "sqd_listed_scan_kernel<2, 2, 1>": 2, "sqd_listed_scan_kernel<2, 2, 2>": 2, "sqd_listed_scan_kernel<2, 3, 1>": 2, "sqd_listed_scan_kernel<2, 3, 2>": 1,
    "sqd_listed_scan_kernel<2, 4, 1>": 1, "sqd_listed_scan_kernel<2, 4, 2>": 1, "sqd_thr_kernel<0, 1, 1>": 8, "sqd_thr_kernel<0, 1, 2>": 8, "sqd_thr_kernel<0, 2, 1>": 8,
    "sqd_thr_kernel<0, 2, 2>": 8, "sqd_thr_kernel<0, 3, 1>": 5, "sqd_thr_kernel<0, 3, 2>": 5, "sqd_thr_kernel<0, 4, 1>": 4, "sqd_thr_kernel<0, 4, 2>": 4,
    "sqd_thr_kernel<1, 1, 1>": 8, "sqd_thr_kernel<1, 1, 2>": 8, "sqd_thr_kernel<1, 2, 1>": 6, "sqd_thr_kernel<1, 2, 2>": 6, "sqd_thr_kernel<1, 3, 1>": 4,
    "sqd_thr_kernel<1, 3, 2>": 4, "sqd_thr_kernel<1, 4, 1>": 4, "sqd_thr_kernel<1, 4, 2>": 4, "sqd_thr_kernel<2, 1, 1>": 8, "sqd_thr_kernel<2, 1, 2>": 8,
    "sqd_thr_kernel<2, 2, 1>": 5, "sqd_thr_kernel<2, 2, 2>": 5, "sqd_thr_kernel<2, 3, 1>": 4, "sqd_thr_kernel<2, 3, 2>": 4, "sqd_thr_kernel<2, 4, 1>": 4,
    "sqd_thr_kernel<2, 4, 2>": 4,
}


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


def row_of(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(" " + name) or key.endswith("::" + name) or key == name]
    assert len(hit) == 1, (name, len(hit))
    return hit[0]


def test_every_kernel_the_routing_reaches_is_built_and_nothing_else(rows):
    assert sorted(REACHED) == sorted(OCC), "the occupancy table names exactly the kernels the routing reaches"
    for name in REACHED:
        row_of(rows, name)
    built = [key for key in rows if "sqd_" in key or "row_sqnorm_kernel" in key or "prep_queries8_raw_kernel" in key or "filter_slack_kernel" in key]
    assert len(built) == len(REACHED), sorted(built)


@pytest.mark.parametrize("name", REACHED)
def test_no_spill_no_scratch_and_the_occupancy_of_this_build(rows, name):
    r = row_of(rows, name)
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
    assert r["occ"] == OCC[name], (name, r, OCC[name])


def test_names_keep_clear_of_the_earlier_guards(golden_dir):
    assert not [n for n in REACHED if "_l2<" in n or "raw_rows_kernel<" in n]
    parent = [line.rsplit(None, 7)[0].strip() for line in open(os.path.join(golden_dir, "spaces_parent_kernel_report.txt")).read().splitlines()[1:]]
    old = [p.replace("void ", "").replace("codd::", "") for p in parent]
    clash = [(n, p) for n in REACHED for p in old if n.endswith(p) or p.endswith(n)]
    assert not clash, clash


def test_the_filter_pass_keeps_two_waves_per_simd_at_full_batch(rows):
    """sqd_filter_kernel<FILTER, 8> runs beside its dot-product twin's occupancy: the extra epilogue terms cost no wave."""
    assert row_of(rows, "sqd_filter_kernel<0, 8>")["occ"] >= row_of(rows, "gemm_filter_kernel<0, 8, 1, 0>")["occ"]
    assert row_of(rows, "sqd_filter_kernel<1, 8>")["occ"] >= row_of(rows, "gemm_filter_kernel<1, 8, 1, 0>")["occ"]
