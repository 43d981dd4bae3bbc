"""Compile-time guard for the embedder kernel: text_embed_kernel must be built, may neither spill nor use scratch,
keeps eight waves per SIMD, and its static LDS is the 1 KiB of tags DESIGN.md states (the accumulator, dim floats, is dynamic
LDS and not in the compiler's figure).  Adding csrc/text_embed.h may not change any kernel that was there before: the golden
reports of the earlier guards are compared by their own tests.  hipcc's own resource report, shared with the other guards; no GPU."""

import os
import re

import pytest

from tests._kernel_report import report_text, resource_rows

NAME = "codd::text_embed_kernel"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def row():
    hit = [r for key, r in resource_rows().items() if key.endswith(NAME)]
    assert hit, f"{NAME} is not in the resource report"
    return hit[0]


def static_lds() -> int:
    for line in report_text().splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8 and parts[0].strip().endswith(NAME):
            return int(parts[6])
    raise AssertionError(f"{NAME} is not in the resource report")


def test_the_kernel_neither_spills_nor_uses_scratch(row):
    assert row["spill"] == 0 and row["scratch"] == 0 and row["sspill"] == 0, row


def test_the_kernel_keeps_full_occupancy(row):
    """One wave per workgroup and one text per wave: the loads of a short text are hidden by the other waves of the SIMD."""
    assert row["occ"] == 8 and row["vgpr"] <= 64, row


def test_static_lds_is_the_tag_table_design_md_states():
    assert static_lds() == 1024
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("## 19.")[1]
    assert re.search(r"1,024 bytes of static LDS", section), "DESIGN.md §19 states the kernel's static LDS"
    assert "4 · dim bytes of dynamic LDS" in section
