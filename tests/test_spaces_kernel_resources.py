"""Compile-time guard for the kernels of the l2 and ip spaces: every squared-L2 kernel the routing can reach — the
whole-store scan for groups of 1, 4 and 8 queries over rows of 1 .. 4 chunks per lane and its wide form (2-byte rows: 4 queries per
pass at most, 2 with two list slots per lane), the scope and the mask list scans, the keys-to-ranks merge — and raw_rows_kernel,
the ingest and query preparation of both spaces, must be built and may neither spill nor use scratch: these are HBM-streaming
scans, and a spill inside the row loop puts a scratch round trip between the loads in flight and their fmaf chains.  OCC is the
occupancy of each of them in this build (waves per SIMD): a change here is a change of the code or of the compiler and is made on
purpose.  tests/golden/spaces_parent_kernel_report.txt is the parent commit's `python -m codd_query_engine_amd.build --report`
(without its last line): every kernel in it must show an identical line in this build — the metric is a compile-time switch that
defaults to the code as it was, and ip runs the dot-product kernels themselves.  hipcc's own resource report, shared with the
other guards; no GPU."""

import os

import pytest

from tests._kernel_report import report_text, resource_rows

SCANS = [f"scan_topk_l2<{dt}, {nb}, {niter}, {sl}>" for dt in (0, 1, 2) for nb in (1, 4, 8) for niter in (1, 2, 3, 4) for sl in (1, 2)]
WIDE = ([f"scan_topk_wide_l2<0, {nb}, {sl}>" for nb in (1, 4, 8) for sl in (1, 2)]
        + [f"scan_topk_wide_l2<{dt}, {nb}, {sl}>" for dt in (1, 2) for nb, sl in ((1, 1), (1, 2), (4, 1), (2, 2))])
LISTS = [f"{head}_scan_l2<{dt}, {niter}, {sl}>" for head in ("scope", "mask") for dt in (0, 1, 2) for niter in (1, 2, 3, 4, 0) for sl in (1, 2)]
SMALL = ["merge_keys_l2<1>", "merge_keys_l2<2>", "raw_rows_kernel<0>", "raw_rows_kernel<1>", "raw_rows_kernel<2>"]
REACHED = SCANS + WIDE + LISTS + SMALL

OCC = {
    "scan_topk_l2<0, 1, 1, 1>": 7, "scan_topk_l2<0, 1, 1, 2>": 7, "scan_topk_l2<0, 1, 2, 1>": 5, "scan_topk_l2<0, 1, 2, 2>": 5, "scan_topk_l2<0, 1, 3, 1>": 4, "scan_topk_l2<0, 1, 3, 2>": 4,
    "scan_topk_l2<0, 1, 4, 1>": 4, "scan_topk_l2<0, 1, 4, 2>": 4, "scan_topk_l2<0, 4, 1, 1>": 5, "scan_topk_l2<0, 4, 1, 2>": 5, "scan_topk_l2<0, 4, 2, 1>": 4, "scan_topk_l2<0, 4, 2, 2>": 3,
    "scan_topk_l2<0, 4, 3, 1>": 3, "scan_topk_l2<0, 4, 3, 2>": 3, "scan_topk_l2<0, 4, 4, 1>": 2, "scan_topk_l2<0, 4, 4, 2>": 2, "scan_topk_l2<0, 8, 1, 1>": 4, "scan_topk_l2<0, 8, 1, 2>": 3,
    "scan_topk_l2<0, 8, 2, 1>": 2, "scan_topk_l2<0, 8, 2, 2>": 2, "scan_topk_l2<0, 8, 3, 1>": 2, "scan_topk_l2<0, 8, 3, 2>": 2, "scan_topk_l2<0, 8, 4, 1>": 1, "scan_topk_l2<0, 8, 4, 2>": 1,
    "scan_topk_l2<1, 1, 1, 1>": 5, "scan_topk_l2<1, 1, 1, 2>": 5, "scan_topk_l2<1, 1, 2, 1>": 4, "scan_topk_l2<1, 1, 2, 2>": 4, "scan_topk_l2<1, 1, 3, 1>": 3, "scan_topk_l2<1, 1, 3, 2>": 3,
    "scan_topk_l2<1, 1, 4, 1>": 2, "scan_topk_l2<1, 1, 4, 2>": 2, "scan_topk_l2<1, 4, 1, 1>": 4, "scan_topk_l2<1, 4, 1, 2>": 3, "scan_topk_l2<1, 4, 2, 1>": 2, "scan_topk_l2<1, 4, 2, 2>": 2,
    "scan_topk_l2<1, 4, 3, 1>": 2, "scan_topk_l2<1, 4, 3, 2>": 1, "scan_topk_l2<1, 4, 4, 1>": 1, "scan_topk_l2<1, 4, 4, 2>": 1, "scan_topk_l2<1, 8, 1, 1>": 3, "scan_topk_l2<1, 8, 1, 2>": 2,
    "scan_topk_l2<1, 8, 2, 1>": 1, "scan_topk_l2<1, 8, 2, 2>": 1, "scan_topk_l2<1, 8, 3, 1>": 1, "scan_topk_l2<1, 8, 3, 2>": 1, "scan_topk_l2<1, 8, 4, 1>": 1, "scan_topk_l2<1, 8, 4, 2>": 1,
    "scan_topk_l2<2, 1, 1, 1>": 5, "scan_topk_l2<2, 1, 1, 2>": 5, "scan_topk_l2<2, 1, 2, 1>": 4, "scan_topk_l2<2, 1, 2, 2>": 4, "scan_topk_l2<2, 1, 3, 1>": 3, "scan_topk_l2<2, 1, 3, 2>": 3,
    "scan_topk_l2<2, 1, 4, 1>": 2, "scan_topk_l2<2, 1, 4, 2>": 2, "scan_topk_l2<2, 4, 1, 1>": 4, "scan_topk_l2<2, 4, 1, 2>": 3, "scan_topk_l2<2, 4, 2, 1>": 2, "scan_topk_l2<2, 4, 2, 2>": 2,
    "scan_topk_l2<2, 4, 3, 1>": 2, "scan_topk_l2<2, 4, 3, 2>": 1, "scan_topk_l2<2, 4, 4, 1>": 1, "scan_topk_l2<2, 4, 4, 2>": 1, "scan_topk_l2<2, 8, 1, 1>": 3, "scan_topk_l2<2, 8, 1, 2>": 2,
    "scan_topk_l2<2, 8, 2, 1>": 1, "scan_topk_l2<2, 8, 2, 2>": 1, "scan_topk_l2<2, 8, 3, 1>": 1, "scan_topk_l2<2, 8, 3, 2>": 1, "scan_topk_l2<2, 8, 4, 1>": 1, "scan_topk_l2<2, 8, 4, 2>": 1,
    "scan_topk_wide_l2<0, 1, 1>": 3, "scan_topk_wide_l2<0, 1, 2>": 3, "scan_topk_wide_l2<0, 4, 1>": 2, "scan_topk_wide_l2<0, 4, 2>": 2, "scan_topk_wide_l2<0, 8, 1>": 2, "scan_topk_wide_l2<0, 8, 2>": 2,
    "scan_topk_wide_l2<1, 1, 1>": 2, "scan_topk_wide_l2<1, 1, 2>": 2, "scan_topk_wide_l2<1, 2, 2>": 2, "scan_topk_wide_l2<1, 4, 1>": 2, "scan_topk_wide_l2<2, 1, 1>": 2, "scan_topk_wide_l2<2, 1, 2>": 2,
    "scan_topk_wide_l2<2, 2, 2>": 2, "scan_topk_wide_l2<2, 4, 1>": 2,
    "scope_scan_l2<0, 0, 1>": 2, "scope_scan_l2<0, 0, 2>": 2, "scope_scan_l2<0, 1, 1>": 4, "scope_scan_l2<0, 1, 2>": 4, "scope_scan_l2<0, 2, 1>": 3, "scope_scan_l2<0, 2, 2>": 3,
    "scope_scan_l2<0, 3, 1>": 2, "scope_scan_l2<0, 3, 2>": 2, "scope_scan_l2<0, 4, 1>": 2, "scope_scan_l2<0, 4, 2>": 1, "scope_scan_l2<1, 0, 1>": 2, "scope_scan_l2<1, 0, 2>": 2,
    "scope_scan_l2<1, 1, 1>": 3, "scope_scan_l2<1, 1, 2>": 3, "scope_scan_l2<1, 2, 1>": 2, "scope_scan_l2<1, 2, 2>": 2, "scope_scan_l2<1, 3, 1>": 1, "scope_scan_l2<1, 3, 2>": 1,
    "scope_scan_l2<1, 4, 1>": 1, "scope_scan_l2<1, 4, 2>": 1, "scope_scan_l2<2, 0, 1>": 2, "scope_scan_l2<2, 0, 2>": 2, "scope_scan_l2<2, 1, 1>": 3, "scope_scan_l2<2, 1, 2>": 3,
    "scope_scan_l2<2, 2, 1>": 2, "scope_scan_l2<2, 2, 2>": 2, "scope_scan_l2<2, 3, 1>": 1, "scope_scan_l2<2, 3, 2>": 1, "scope_scan_l2<2, 4, 1>": 1, "scope_scan_l2<2, 4, 2>": 1,
    "mask_scan_l2<0, 0, 1>": 2, "mask_scan_l2<0, 0, 2>": 2, "mask_scan_l2<0, 1, 1>": 5, "mask_scan_l2<0, 1, 2>": 4, "mask_scan_l2<0, 2, 1>": 3, "mask_scan_l2<0, 2, 2>": 3,
    "mask_scan_l2<0, 3, 1>": 2, "mask_scan_l2<0, 3, 2>": 2, "mask_scan_l2<0, 4, 1>": 2, "mask_scan_l2<0, 4, 2>": 2, "mask_scan_l2<1, 0, 1>": 2, "mask_scan_l2<1, 0, 2>": 2,
    "mask_scan_l2<1, 1, 1>": 4, "mask_scan_l2<1, 1, 2>": 4, "mask_scan_l2<1, 2, 1>": 2, "mask_scan_l2<1, 2, 2>": 2, "mask_scan_l2<1, 3, 1>": 2, "mask_scan_l2<1, 3, 2>": 2,
    "mask_scan_l2<1, 4, 1>": 2, "mask_scan_l2<1, 4, 2>": 2, "mask_scan_l2<2, 0, 1>": 2, "mask_scan_l2<2, 0, 2>": 2, "mask_scan_l2<2, 1, 1>": 4, "mask_scan_l2<2, 1, 2>": 4,
    "mask_scan_l2<2, 2, 1>": 2, "mask_scan_l2<2, 2, 2>": 2, "mask_scan_l2<2, 3, 1>": 2, "mask_scan_l2<2, 3, 2>": 2, "mask_scan_l2<2, 4, 1>": 2, "mask_scan_l2<2, 4, 2>": 2,
    "merge_keys_l2<1>": 8, "merge_keys_l2<2>": 8, "raw_rows_kernel<0>": 8, "raw_rows_kernel<1>": 8, "raw_rows_kernel<2>": 8,
}


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


def row_of(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(" " + name) or key == name]
    assert len(hit) == 1, (name, len(hit))
    return hit[0]


def test_every_kernel_the_routing_reaches_is_built_and_nothing_else(rows):
    assert sorted(REACHED) == sorted(OCC), "the occupancy table names exactly the kernels the routing reaches"
    for name in REACHED:
        row_of(rows, name)
    built = [key for key in rows if "_l2<" in key or "raw_rows_kernel<" in key]
    assert len(built) == len(REACHED), sorted(set(k.replace("void ", "") for k in built) - set(REACHED))


@pytest.mark.parametrize("name", REACHED)
def test_no_spill_no_scratch_and_the_occupancy_of_this_build(rows, name):
    r = row_of(rows, name)
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
    assert r["occ"] == OCC[name], (name, r, OCC[name])


def test_new_names_end_in_no_existing_kernels_name(golden_dir):
    """The guards of earlier commits look kernels up with key.endswith("scan_topk_kernel<0, 1, 3, 1>") and the like."""
    parent = [line.rsplit(None, 7)[0].strip() for line in open(os.path.join(golden_dir, "spaces_parent_kernel_report.txt")).read().splitlines()[1:]]
    old = [p.replace("void ", "").replace("codd::", "") for p in parent]
    clash = [(n, p) for n in REACHED for p in old if n.endswith(p) or p.endswith(n)]
    assert not clash, clash


def table(text: str) -> dict:
    out = {}
    for line in text.splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8:
            out[parts[0].strip()] = parts[1:]
    return out


def test_every_kernel_of_the_parent_build_shows_an_identical_report(golden_dir):
    """A guard of the commit that added the spaces: the golden file is the report of the build before it, by the compiler of that
    day.  A later change that touches one of those kernels on purpose, or a compiler update, re-baselines it or retires this test."""
    parent = table(open(os.path.join(golden_dir, "spaces_parent_kernel_report.txt")).read())
    mine = table(report_text())
    assert len(parent) > 370
    assert not [n for n in parent if n not in mine], "a kernel of the parent build is gone"
    differ = {n: (parent[n], mine[n]) for n in parent if parent[n] != mine[n]}
    assert not differ, differ


def test_the_l2_scans_keep_the_occupancy_of_the_dot_product_scans_where_the_bytes_are(rows):
    """f32 rows (the flagship storage): the extra subtraction per element costs no wave per SIMD in the whole-store scan."""
    for name in SCANS + WIDE:
        if not name.startswith(("scan_topk_l2<0,", "scan_topk_wide_l2<0,")):
            continue
        twin = name.replace("scan_topk_l2<", "scan_topk_kernel<").replace("scan_topk_wide_l2<", "scan_topk_wide_kernel<")
        assert row_of(rows, name)["occ"] >= row_of(rows, twin)["occ"], (name, twin)
