"""Compile-time guard for scope_scan_kernel, the row-gathering scan behind namespace-scoped search: every
instantiation the dispatch can reach — three storage dtypes, 1 .. 4 chunks per lane and the wide form (NITER 0), one or two list
slots per lane — must be built, and none may spill: a spill inside the row loop would put a scratch round trip between the
gathered loads and their fmaf chains.  Same recipe as tests/test_kernel_resources.py: hipcc's own resource report, no GPU."""

import re
import subprocess

import pytest

from codd_query_engine_amd import build as b


@pytest.fixture(scope="module")
def rows():
    cmd = [b._hipcc(), *[f for f in b.HIPCC_FLAGS if f != "-shared"], "-c", "-I", b.os.path.join(b._ROOT, "include"), "-I", b.CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", b.os.path.join(b.CSRC, b.SOURCES[0])]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    out = {}
    for line in b.resource_report(proc.stderr).splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\S+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            out[m.group(1).strip()] = {"vgpr": int(m.group(2)), "spill": int(m.group(4)), "scratch": int(m.group(5)), "occ": int(m.group(6)),
                                       "sspill": int(m.group(8))}
    return out


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


def test_scope_list_builders_are_built_and_tiny(rows):
    for kern in ("scope_set_kernel", "scope_count_kernel", "scope_offsets_kernel", "scope_scatter_kernel", "scope_group_kernel"):
        hit = [r for key, r in rows.items() if key.endswith(kern)]
        assert hit, kern
        assert hit[0]["scratch"] == 0 and hit[0]["spill"] == 0 and hit[0]["sspill"] == 0, (kern, hit[0])
