"""Compile-time guard for the document kernels: doc_match_kernel and mask_clip_count_kernel must be built and may
neither spill nor use scratch — the needle travels as a kernel argument and is indexed by the thread id, which must stay a load
from the argument segment, not a private copy — and every kernel of the build before them must show the report it showed then
(tests/golden/documents_parent_kernel_report.txt: that build's `python -m codd_query_engine_amd.build --report`): the host-mask
entry point and the unmasked searches launch what they launched.  hipcc's own resource report, shared with the other guards; no GPU."""

import os

import pytest

from tests._kernel_report import report_text, resource_rows

NEW = ["codd::doc_match_kernel", "codd::mask_clip_count_kernel"]


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
def test_the_document_kernels_are_built_and_neither_spill_nor_use_scratch(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    assert hit[0]["spill"] == 0 and hit[0]["scratch"] == 0 and hit[0]["sspill"] == 0, (name, hit[0])


def test_the_match_kernel_keeps_full_occupancy(rows):
    """A streaming kernel with one LDS tile per workgroup hides its loads behind other workgroups: eight waves per SIMD."""
    r = [r for key, r in rows.items() if key.endswith(NEW[0])][0]
    assert r["occ"] == 8, r


def test_every_kernel_of_the_parent_build_shows_an_identical_report(golden_dir):
    """A guard of the commit that added the document kernels: the golden file is the report of the build before it, by the
    compiler of that day.  A later change that touches one of those kernels on purpose, or a compiler update, re-baselines it
    (`python -m codd_query_engine_amd.build --report`, without the last line) or retires this test; kernels that are not in the
    golden file are nobody's business here."""
    parent = table(open(os.path.join(golden_dir, "documents_parent_kernel_report.txt")).read())
    mine = table(report_text())
    assert len(parent) > 300
    assert not [n for n in parent if n not in mine], "a kernel of the parent build is gone"
    differ = {n: (parent[n], mine[n]) for n in parent if parent[n] != mine[n]}
    assert not differ, differ
