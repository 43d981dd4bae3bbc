"""Compile-time guard for the regular-expression kernel: doc_regex_kernel must be built, may neither spill nor use
scratch, and keeps the occupancy its LDS budget was chosen for — a segment of 8,192 bytes beside the class map and a table of up to
8,192 bytes, so that eight workgroups share a compute unit.  hipcc's own resource report, shared with the other guards; no GPU."""

import pytest

from tests._kernel_report import resource_rows

NAME = "codd::doc_regex_kernel"


@pytest.fixture(scope="module")
def row():
    hit = [r for key, r in resource_rows().items() if key.endswith(NAME)]
    assert hit, NAME + " is not in the build"
    return hit[0]


def test_the_kernel_is_built_and_neither_spills_nor_uses_scratch(row):
    assert row["spill"] == 0 and row["scratch"] == 0 and row["sspill"] == 0, row


def test_the_kernel_keeps_eight_waves_per_simd(row):
    """A lane waits on dependent LDS reads (document word, class, table entry): other waves fill the time."""
    assert row["occ"] == 8, row
