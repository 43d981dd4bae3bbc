"""Compile-time guard for the predicate kernel: where_eval_kernel must be built and may neither spill nor use
scratch — its program arrives by value and is indexed with wave-uniform values only, so nothing of it may end up in private memory.
The two column kernels beside it are held to the same.  hipcc's own resource report, shared with the other guards; no GPU."""

import pytest

from tests._kernel_report import resource_rows

NAMES = ["codd::where_eval_kernel", "codd::column_set_kernel", "codd::column_compact_kernel"]


@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_is_built_and_neither_spills_nor_uses_scratch(name):
    hit = [r for key, r in resource_rows().items() if key.endswith(name)]
    assert hit, name + " is not in the build"
    row = hit[0]
    assert row["spill"] == 0 and row["scratch"] == 0 and row["sspill"] == 0, row


def test_the_predicate_kernel_keeps_eight_waves_per_simd():
    """A pure stream: its loads are hidden by other waves, so the register budget must leave room for all eight."""
    row = [r for key, r in resource_rows().items() if key.endswith(NAMES[0])][0]
    assert row["occ"] == 8, row
