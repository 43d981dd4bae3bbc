"""Compile-time guard for the kernels of masked search: the deny launch, the two list builders and every
instantiation of mask_scan_kernel the dispatch can reach — three storage dtypes, 1 .. 4 chunks per lane (the 2-byte rows of four
chunks take two queries per work item) and the wide form (NITER 0), one or two list slots per lane — must be built, and none
may spill or use scratch: a spill inside the row loop would put a scratch round trip between the gathered loads and their fmaf
chains.  hipcc's own resource report, shared with the other guards; no GPU."""

import pytest

from tests._kernel_report import resource_rows


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


SCANS = [f"mask_scan_kernel<{dt}, {niter}, {sl}>" for dt in (0, 1, 2) for niter in (1, 2, 3, 4, 0) for sl in (1, 2)]
SMALL = ["mask_deny_kernel", "mask_prefix_kernel", "mask_scatter_kernel"]


def test_every_masked_kernel_is_built(rows):
    missing = [n for n in SCANS + SMALL if not any(name.endswith(n) for name in rows)]
    assert not missing, missing


@pytest.mark.parametrize("name", SCANS + SMALL)
def test_masked_kernels_neither_spill_nor_use_scratch(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    r = hit[0]
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)


def test_the_mask_scan_is_no_heavier_than_the_scope_scan_it_mirrors(rows):
    """The same list_scan_body under a simpler head: at least the occupancy of scope_scan_kernel's instantiation."""
    for name in SCANS:
        mine = [r for key, r in rows.items() if key.endswith(name)][0]
        theirs = [r for key, r in rows.items() if key.endswith(name.replace("mask_scan", "scope_scan"))][0]
        assert mine["occ"] >= theirs["occ"], (name, mine, theirs)
