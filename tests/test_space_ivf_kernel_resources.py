"""Compile-time guard for the list scans of an l2 index's IVF: every squared-L2 IVF scan the routing can reach — the
per-pair scan `ivf_scan_sq` for rows of 1 .. 4 chunks per lane and the wide form, the list-sharing scan `ivf_shared_sq` for the same
rows except 2-byte rows of 4 chunks per lane (which never take the shared scan, as under cosine), one and two list slots each — must
be built, and nothing else under those names, and none may spill, use scratch or spill an SGPR.  OCC is the occupancy of each in
this build (waves per SIMD): a change is a change of the code or of the compiler and is made on purpose.  The names keep clear of the
guards of earlier commits, and tests/golden/space_ivf_parent_kernel_report.txt is the parent commit's
`python -m codd_query_engine_amd.build --report` (without its last line): every kernel in it must show an identical line in this
build — ip runs the dot-product list scans themselves, and the l2 scans are kernels of their own beside them.  hipcc's own resource
report, shared with the other guards; no GPU."""

import os

import pytest

from tests._kernel_report import report_text, resource_rows

FORMS = [(dt, niter, sl) for dt in (0, 1, 2) for niter in (1, 2, 3, 4, 0) for sl in (1, 2)]
PAIR = [f"ivf_scan_sq<{dt}, {niter}, {sl}>" for dt, niter, sl in FORMS]
SHARED = [f"ivf_shared_sq<{dt}, {niter}, {sl}>" for dt, niter, sl in FORMS if not (dt != 0 and niter == 4)]
REACHED = PAIR + SHARED

OCC = {
    "ivf_scan_sq<0, 0, 1>": 4, "ivf_scan_sq<0, 0, 2>": 4, "ivf_scan_sq<0, 1, 1>": 8, "ivf_scan_sq<0, 1, 2>": 8, "ivf_scan_sq<0, 2, 1>": 7,
    "ivf_scan_sq<0, 2, 2>": 6, "ivf_scan_sq<0, 3, 1>": 5, "ivf_scan_sq<0, 3, 2>": 5, "ivf_scan_sq<0, 4, 1>": 4, "ivf_scan_sq<0, 4, 2>": 4,
    "ivf_scan_sq<1, 0, 1>": 2, "ivf_scan_sq<1, 0, 2>": 2, "ivf_scan_sq<1, 1, 1>": 8, "ivf_scan_sq<1, 1, 2>": 8, "ivf_scan_sq<1, 2, 1>": 6,
    "ivf_scan_sq<1, 2, 2>": 5, "ivf_scan_sq<1, 3, 1>": 4, "ivf_scan_sq<1, 3, 2>": 4, "ivf_scan_sq<1, 4, 1>": 3, "ivf_scan_sq<1, 4, 2>": 3,
    "ivf_scan_sq<2, 0, 1>": 2, "ivf_scan_sq<2, 0, 2>": 2, "ivf_scan_sq<2, 1, 1>": 8, "ivf_scan_sq<2, 1, 2>": 8, "ivf_scan_sq<2, 2, 1>": 6,
    "ivf_scan_sq<2, 2, 2>": 5, "ivf_scan_sq<2, 3, 1>": 4, "ivf_scan_sq<2, 3, 2>": 4, "ivf_scan_sq<2, 4, 1>": 3, "ivf_scan_sq<2, 4, 2>": 3,
    "ivf_shared_sq<0, 0, 1>": 2, "ivf_shared_sq<0, 0, 2>": 2, "ivf_shared_sq<0, 1, 1>": 5, "ivf_shared_sq<0, 1, 2>": 5, "ivf_shared_sq<0, 2, 1>": 3,
    "ivf_shared_sq<0, 2, 2>": 3, "ivf_shared_sq<0, 3, 1>": 2, "ivf_shared_sq<0, 3, 2>": 2, "ivf_shared_sq<0, 4, 1>": 2, "ivf_shared_sq<0, 4, 2>": 2,
    "ivf_shared_sq<1, 0, 1>": 2, "ivf_shared_sq<1, 0, 2>": 2, "ivf_shared_sq<1, 1, 1>": 4, "ivf_shared_sq<1, 1, 2>": 4, "ivf_shared_sq<1, 2, 1>": 3,
    "ivf_shared_sq<1, 2, 2>": 2, "ivf_shared_sq<1, 3, 1>": 2, "ivf_shared_sq<1, 3, 2>": 2, "ivf_shared_sq<2, 0, 1>": 2, "ivf_shared_sq<2, 0, 2>": 2,
    "ivf_shared_sq<2, 1, 1>": 4, "ivf_shared_sq<2, 1, 2>": 4, "ivf_shared_sq<2, 2, 1>": 3, "ivf_shared_sq<2, 2, 2>": 2, "ivf_shared_sq<2, 3, 1>": 2,
    "ivf_shared_sq<2, 3, 2>": 2,
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
    built = [key for key in rows if "ivf_scan_sq" in key or "ivf_shared_sq" in key]
    assert len(built) == len(REACHED) == 56, sorted(set(k.replace("void ", "") for k in built) - set(REACHED))


@pytest.mark.parametrize("name", REACHED)
def test_no_spill_no_scratch_and_the_occupancy_of_this_build(rows, name):
    r = row_of(rows, name)
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
    assert r["occ"] == OCC[name], (name, r, OCC[name])


def test_the_f32_forms_keep_the_occupancy_of_their_dot_product_twins(rows):
    for name in REACHED:
        if not name.startswith(("ivf_scan_sq<0,", "ivf_shared_sq<0,")):
            continue
        twin = name.replace("ivf_scan_sq<", "ivf_scan_kernel<").replace("ivf_shared_sq<", "ivf_scan_shared_kernel<")
        assert row_of(rows, name)["occ"] >= row_of(rows, twin)["occ"], (name, row_of(rows, name), twin, row_of(rows, twin))


def table(text: str) -> dict:
    out = {}
    for line in text.splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8:
            out[parts[0].strip()] = parts[1:]
    return out


def test_names_keep_clear_of_the_earlier_guards(golden_dir):
    counted = ("_l2<", "raw_rows_kernel<", "sqd_", "row_sqnorm_kernel", "prep_queries8_raw_kernel", "filter_slack_kernel")
    assert not [n for n in REACHED if any(c in n for c in counted)]
    parent = table(open(os.path.join(golden_dir, "space_ivf_parent_kernel_report.txt")).read())
    old = [p.replace("void ", "").replace("codd::", "") for p in parent]
    clash = [(n, p) for n in REACHED for p in old if n.endswith(p) or p.endswith(n)]
    assert not clash, clash


def test_every_kernel_of_the_parent_build_shows_an_identical_report(golden_dir):
    """A guard of the commit that added IVF for ip and l2: the golden file is the report of the build before it, by the compiler of
    that day.  A later change that touches one of those kernels on purpose, or a compiler update, re-baselines it or retires this
    test."""
    parent = table(open(os.path.join(golden_dir, "space_ivf_parent_kernel_report.txt")).read())
    mine = table(report_text())
    assert len(parent) > 600
    assert not [n for n in parent if n not in mine], "a kernel of the parent build is gone"
    differ = {n: (parent[n], mine[n]) for n in parent if parent[n] != mine[n]}
    assert not differ, differ


def test_the_committed_table_is_this_build_s():
    """profiles/space_ivf/kernel_resources.txt keeps the lines of the new kernels and of their dot-product twins."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kept = table(open(os.path.join(root, "profiles", "space_ivf", "kernel_resources.txt")).read())
    mine = table(report_text())
    assert all(any(key.endswith(n) for key in kept) for n in REACHED)
    assert not {n: (kept[n], mine.get(n)) for n in kept if kept[n] != mine.get(n)}
