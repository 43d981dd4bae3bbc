"""Compile-time guard for scope_scan_kernel, the row-gathering scan behind namespace-scoped search: every
instantiation the dispatch can reach — three storage dtypes, 1 .. 4 chunks per lane and the wide form (NITER 0), one or two list
slots per lane — must be built, and none may spill: a spill inside the row loop would put a scratch round trip between the
gathered loads and their fmaf chains.  Same recipe as tests/test_kernel_resources.py: hipcc's own resource report, no GPU."""

import pytest

from tests._kernel_report import resource_rows


@pytest.fixture(scope="module")
def rows():
    return resource_rows()


NAMES = [f"scope_scan_kernel<{dt}, {niter}, {sl}>" for dt in (0, 1, 2) for niter in (1, 2, 3, 4, 0) for sl in (1, 2)]


def test_every_scope_scan_instantiation_is_built(rows):
    missing = [n for n in NAMES if not any(name.endswith(n) for name in rows)]
    assert not missing, missing


@pytest.mark.parametrize("name", NAMES)
def test_scope_scan_neither_spills_nor_uses_scratch(rows, name):
    hit = [r for key, r in rows.items() if key.endswith(name)]
    assert hit, name
    r = hit[0]
    assert r["spill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)


# occupancy (waves per SIMD) of every instantiation in the build before the list-driven scan body was shared with the IVF scan, from
# that build's own report
PARENT_OCC = {
    "scope_scan_kernel<0, 1, 1>": 4, "scope_scan_kernel<0, 1, 2>": 4, "scope_scan_kernel<0, 2, 1>": 3, "scope_scan_kernel<0, 2, 2>": 3, "scope_scan_kernel<0, 3, 1>": 2,
    "scope_scan_kernel<0, 3, 2>": 2, "scope_scan_kernel<0, 4, 1>": 2, "scope_scan_kernel<0, 4, 2>": 2, "scope_scan_kernel<0, 0, 1>": 2, "scope_scan_kernel<0, 0, 2>": 2,
    "scope_scan_kernel<1, 1, 1>": 3, "scope_scan_kernel<1, 1, 2>": 3, "scope_scan_kernel<1, 2, 1>": 2, "scope_scan_kernel<1, 2, 2>": 2, "scope_scan_kernel<1, 3, 1>": 1,
    "scope_scan_kernel<1, 3, 2>": 1, "scope_scan_kernel<1, 4, 1>": 1, "scope_scan_kernel<1, 4, 2>": 1, "scope_scan_kernel<1, 0, 1>": 2, "scope_scan_kernel<1, 0, 2>": 2,
    "scope_scan_kernel<2, 1, 1>": 3, "scope_scan_kernel<2, 1, 2>": 3, "scope_scan_kernel<2, 2, 1>": 2, "scope_scan_kernel<2, 2, 2>": 2, "scope_scan_kernel<2, 3, 1>": 1,
    "scope_scan_kernel<2, 3, 2>": 1, "scope_scan_kernel<2, 4, 1>": 1, "scope_scan_kernel<2, 4, 2>": 1, "scope_scan_kernel<2, 0, 1>": 2, "scope_scan_kernel<2, 0, 2>": 2,
}


def test_scope_scan_keeps_its_occupancy(rows):
    assert set(PARENT_OCC) == set(NAMES)
    occ = {}
    for name in NAMES:
        hit = [r for key, r in rows.items() if key.endswith(name)]
        assert hit, name
        occ[name] = hit[0]["occ"]
    worse = [(name, occ[name], PARENT_OCC[name]) for name in NAMES if occ[name] < PARENT_OCC[name]]
    assert not worse, worse


def test_scope_list_builders_are_built_and_tiny(rows):
    for kern in ("scope_set_kernel", "scope_count_kernel", "scope_offsets_kernel", "scope_scatter_kernel", "scope_group_kernel"):
        hit = [r for key, r in rows.items() if key.endswith(kern)]
        assert hit, kern
        assert hit[0]["scratch"] == 0 and hit[0]["spill"] == 0 and hit[0]["sspill"] == 0, (kern, hit[0])
