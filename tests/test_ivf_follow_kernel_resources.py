"""Compile-time guard for the kernels of an IVF layout that follows writes: every new kernel must be built — the delta
scan in every row form the IVF scans have — and may neither spill nor use scratch; the committed table is this build's.  The existing
kernels take no new argument (the delta's partial keys reach the merge through its run arguments), which the guards of the earlier
builds' reports hold.  hipcc's own resource report, shared with the other guards; no GPU."""

import os

import pytest

from tests._kernel_report import report_text, resource_rows

SMALL = ["pend_set_kernel", "pend_or_kernel", "list_of_build_kernel", "list_assign_kernel", "ivf_list_count_kernel", "ivf_list_offsets_kernel",
         "ivf_list_scatter_kernel"]
# (dtype, NITER, SLOTS): f32 / bf16 / f16 rows of 1 .. 4 chunks per lane and the wide form (0), one and two list slots per lane
FORMS = [(dt, ni, sl) for dt in (0, 1, 2) for ni in (1, 2, 3, 4, 0) for sl in (1, 2)]


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


def table(text: str) -> dict:
    out = {}
    for line in text.splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8:
            out[parts[0].strip()] = parts[1:]
    return out


def clean(row):
    return row["spill"] == 0 and row["scratch"] == 0 and row["sspill"] == 0


@pytest.mark.parametrize("name", SMALL)
def test_the_bookkeeping_and_fold_kernels_are_built_and_clean(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    assert clean(hit[0]) and hit[0]["occ"] == 8, (name, hit[0])      # a word or a row slot per thread: nothing should hold the occupancy down


def test_the_delta_scan_is_built_in_every_row_form_and_never_spills(rows):
    for kernel in ("ivf_delta_kernel", "ivf_delta_sq"):
        for dt, ni, sl in FORMS:
            name = f"{kernel}<{dt}, {ni}, {sl}>"
            hit = [r for key, r in rows.items() if key.endswith(name)]
            assert hit, name
            assert clean(hit[0]) and hit[0]["occ"] >= 2, (name, hit[0])
    for dt in (0, 1, 2):
        hit = [r for key, r in rows.items() if key.endswith(f"widen_listed_rows_kernel<{dt}>")]
        assert hit and clean(hit[0]), dt


def test_the_committed_table_is_this_build_s():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kept = table(open(os.path.join(root, "profiles", "ivf_follow", "kernel_resources.txt")).read())
    mine = table(report_text())
    assert len(kept) == len(SMALL) + 3 + 2 * len(FORMS)
    assert not {n: (kept[n], mine.get(n)) for n in kept if kept[n] != mine.get(n)}
