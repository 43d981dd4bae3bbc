"""Compile-time guard for the masked IVF and sharded routes: mask_slice_kernel must be built and may neither spill
nor use scratch, and every kernel of the build before it must show the report it showed then
(tests/golden/ivf_masked_parent_kernel_report.txt: that build's `python -m codd_query_engine_amd.build --report`) — the masked IVF
entry points pass another bitmap to the list scans that exist; no existing kernel changes.  hipcc's own resource report, shared with
the other guards; no GPU."""

import os

import pytest

from tests._kernel_report import report_text, resource_rows

NEW = ["codd::mask_slice_kernel"]


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


def table(text: str) -> dict:
    """kernel name -> the columns of its line, as printed."""
    out = {}
    for line in text.splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8:
            out[parts[0].strip()] = parts[1:]
    return out


@pytest.mark.parametrize("name", NEW)
def test_the_slicing_kernel_is_built_and_neither_spills_nor_uses_scratch(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    assert hit[0]["spill"] == 0 and hit[0]["scratch"] == 0 and hit[0]["sspill"] == 0, (name, hit[0])
    assert hit[0]["occ"] == 8, hit[0]          # one word per thread, no LDS: nothing should hold the occupancy down


def test_every_kernel_of_the_parent_build_shows_an_identical_report(golden_dir):
    """A guard of the commit that added the masked IVF and sharded routes: the golden file is the report of the build before it, by
    the compiler of that day.  A later change that touches one of those kernels on purpose, or a compiler update, re-baselines it
    (`python -m codd_query_engine_amd.build --report`, without the last line) or retires this test; kernels that are not in the
    golden file are nobody's business here."""
    parent = table(open(os.path.join(golden_dir, "ivf_masked_parent_kernel_report.txt")).read())
    mine = table(report_text())
    assert len(parent) > 300
    assert not [n for n in parent if n not in mine], "a kernel of the parent build is gone"
    differ = {n: (parent[n], mine[n]) for n in parent if parent[n] != mine[n]}
    assert not differ, differ


def test_the_committed_table_is_this_build_s(rows):
    """profiles/ivf_masked/kernel_resources.txt keeps the new kernel's line and the lines of the kernels the masked IVF route launches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kept = table(open(os.path.join(root, "profiles", "ivf_masked", "kernel_resources.txt")).read())
    mine = table(report_text())
    assert any(n.endswith(NEW[0]) for n in kept)
    assert not {n: (kept[n], mine.get(n)) for n in kept if kept[n] != mine.get(n)}
