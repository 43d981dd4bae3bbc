"""The plan of the six-interval int8 tile programs (csrc/geometry.h: sweep_*) without a device, through
tests/host/sweep_plan_main.cpp compiled with the library's compiler as a plain host compiler.

The host program walks a workgroup's tiles with a model of the four LDS slots of the query block, of the three register slots of
the corpus ring and of the wave's in-order vector-memory queue, and exits non-zero at the first violation:
  * every computed K-step reads a slot that holds that step's slice, landed (this wave's wait) at or before the preceding barrier;
  * no slot is overwritten before the barrier that follows its last read;
  * each tile covers K-steps {0..5} exactly once, from ring slots that hold that tile's and that step's fragments;
  * every vmcnt the constexpr functions yield equals the model's count of younger operations at that wait.
The kernel takes its steps, slots and waits from the same functions (static_assert where it folds them into constants)."""

from __future__ import annotations

import os
import subprocess

import pytest

from codd_query_engine_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (1, 2, 3, 7)
EARLY = (0, 1, 2, 3)   # every CODD_I8_EARLY_A mask; 3 is what ships
DPS = 4                # slice DMA per wave and slice at 16 query blocks (NQB / 4)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_plan") / "sweep_plan_main")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", build.CSRC, "-I", build.INCLUDE,
           os.path.join(ROOT, "tests", "host", "sweep_plan_main.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "geometry.h does not compile as plain C++17 without HIP:\n" + proc.stdout + proc.stderr
    return exe


def walk(program, sweep, tiles, early, dps=DPS, bug=0, where=0):
    proc = subprocess.run([program, *map(str, (sweep, tiles, early, dps, bug, where))], capture_output=True, text=True)
    return proc.returncode, proc.stdout.strip()


@pytest.mark.parametrize("tiles", TILES)
def test_the_sweep_holds_for_every_workgroup_size_and_early_mask(program, tiles):
    for early in EARLY:
        # four slices once in the prologue, two per tile — odd tile counts end on a forward tile with no special case
        assert walk(program, 1, tiles, early) == (0, f"ok 4 2 {tiles}"), (tiles, early)
        assert walk(program, 1, tiles, early, dps=2) == (0, f"ok 4 2 {tiles}"), (tiles, early)


@pytest.mark.parametrize("tiles", TILES)
def test_the_static_program_s_counts_come_from_the_same_walk(program, tiles):
    for early in EARLY:
        assert walk(program, 0, tiles, early) == (0, f"ok 2 6 {tiles}"), (tiles, early)


def test_a_seeded_off_by_one_in_the_slot_rule_fails(program):
    for step in range(6):
        rc, out = walk(program, 1, 3, 3, bug=1, where=step)
        assert rc == 1 and out.startswith("FAIL") and ("slot" in out), (step, out)


def test_a_seeded_off_by_one_in_one_wait_fails(program):
    for interval in range(6):
        for bug in (2, 3):   # one operation too lax, one too strict
            rc, out = walk(program, 1, 3, 3, bug=bug, where=interval)
            assert rc == 1 and "corpus wait" in out, (interval, bug, out)
    # the barrier that hands the staged slices over (interval 3): one operation too lax and a slice has not landed when it is read
    rc, out = walk(program, 1, 3, 3, bug=4, where=3)
    assert rc == 1 and "does not hold its slice" in out, out
