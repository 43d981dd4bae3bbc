"""Compile-time guard for i8_sweep_kernel (csrc/filter_i8.h): hipcc's own resource report, no GPU.  The kernel issues
its loads and LDS-DMA by inline asm that hipcc cannot see in flight, so — like every i8_tile_kernel instantiation
(tests/test_kernel_resources.py) — it may not touch scratch, spill a vector register or park scalar registers in vector lanes, and
it keeps two waves per SIMD.  The static program sits at 106 scalar registers; the direction of a tile must not cost more."""

import os

from tests._kernel_report import report_text, resource_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(text: str) -> dict:
    out = {}
    for line in text.splitlines()[1:]:
        parts = line.rsplit(None, 7)
        if len(parts) == 8:
            out[parts[0].strip()] = parts[1:]
    return out


def test_the_sweep_kernel_is_built_and_does_not_spill():
    rows = resource_rows()
    sweep = [name for name in rows if "i8_sweep_kernel" in name]
    assert len(sweep) == 1 and "i8_sweep_kernel<16, 0, 3, false, false, true>" in sweep[0], sweep   # (NQB, then the fixed MODE_FILTER, TS = 3, staged, int8, sweep)
    assert not [name for name in sweep if "i8_tile_kernel" in name]
    r = rows[sweep[0]]
    assert (r["scratch"], r["spill"], r["sspill"], r["occ"]) == (0, 0, 0, 2), r
    assert r["vgpr"] <= 256
    sgpr = int(table(report_text())[sweep[0]][1])
    assert sgpr <= 106, sgpr


def test_the_committed_table_is_this_build_s():
    """profiles/sweep/kernel_resources.txt keeps the lines of the new kernel and of the static program it is the twin of"""
    kept = table(open(os.path.join(ROOT, "profiles", "sweep", "kernel_resources.txt")).read())
    mine = table(report_text())
    assert any("i8_sweep_kernel<16," in name for name in kept) and any(name.endswith("i8_tile_kernel<0, 3, 16, false, false>") for name in kept)
    assert not {n: (kept[n], mine.get(n)) for n in kept if kept[n] != mine.get(n)}
