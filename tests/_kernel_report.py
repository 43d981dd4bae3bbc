"""hipcc's own resource report of the library, compiled ONCE per test run (no GPU: hipcc cross-compiles for gfx950) and shared
by the compile-time guards: test_kernel_resources, test_wide_kernel_resources, test_scoped_kernel_resources and
test_delete_kernel_resources."""

import functools
import re
import subprocess

from codd_query_engine_amd import build as b


@functools.lru_cache(maxsize=None)
def report_text() -> str:
    """build.resource_report's table: one line per kernel."""
    cmd = [b._hipcc(), *[f for f in b.HIPCC_FLAGS if f != "-shared"], "-c", "-I", b.os.path.join(b._ROOT, "include"), "-I", b.CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null", b.os.path.join(b.CSRC, b.SOURCES[0])]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return b.resource_report(proc.stderr)


@functools.lru_cache(maxsize=None)
def resource_rows() -> dict:
    """kernel name -> {vgpr, spill, scratch, occ, sspill}."""
    out = {}
    for line in report_text().splitlines()[1:]:
        m = re.match(r"(.+?)\s+(\d+)\s+(\S+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            out[m.group(1).strip()] = {"vgpr": int(m.group(2)), "spill": int(m.group(4)), "scratch": int(m.group(5)), "occ": int(m.group(6)),
                                       "sspill": int(m.group(8))}
    return out
