"""The sample cascade's plan (csrc/search_plan.h: cascade_geometry, cascade_plan, cascade_pick_d) without a device,
through tests/host/cascade_plan_main.cpp compiled with the library's compiler as a plain host compiler.

The cascade splits the tiles of a filter pass between two launches of the filter program: A1 takes tiles 0, d + 1, 2 (d + 1), ...,
B every other tile, enumerated per workgroup from (first, step, my_tiles) alone — the same three numbers i8_tile_kernel derives from
its block number, the grid and d.  The two sets must be disjoint and together [0, ntiles); the first sample A0 must avoid A1's
tiles (the re-anchor takes k distinct rows from A0's keys and A1's candidates); d must divide the grid."""

from __future__ import annotations

import os
import subprocess

import pytest

from codd_query_engine_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (1, 7, 64, 256, 304)
D_MIN, D_MAX = 16, 64
TILE, STATIC = 1, 3   # FilterProgram::TILE, its static six-step form


def admissible(G):
    return [d for d in range(D_MIN, D_MAX + 1) if G % d == 0]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cascade_plan") / "cascade_plan_main")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", build.CSRC, "-I", build.INCLUDE,
           os.path.join(ROOT, "tests", "host", "cascade_plan_main.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "search_plan.h does not compile as plain C++17 without HIP:\n" + proc.stdout + proc.stderr
    return exe


def run(program, lines):
    proc = subprocess.run([program], input="".join(" ".join(str(int(v)) for v in line) + "\n" for line in lines), capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return [[int(v) for v in out.split()] for out in proc.stdout.splitlines()]


def test_the_grids_have_the_divisors_the_cases_assume():
    assert [admissible(G) for G in GRIDS] == [[], [], [16, 32, 64], [16, 32, 64], [16, 19, 38]]


def test_a1_and_b_partition_the_tiles_and_a0_avoids_a1(program):
    """every admissible d of every grid, every ntiles from 1 to 3,000 (below the grid, below d + 1, d + 1 itself, no multiple of d + 1,
    several rounds of B), counted tile by tile by the host program"""
    cases = [(G, d) for G in GRIDS for d in admissible(G)]
    got = run(program, [[2, G, d, 1, 3000] for G, d in cases])
    for (G, d), (n, uncovered, twice, a0_in_a1, a0_outside, a0_repeated) in zip(cases, got, strict=True):
        assert (n, uncovered, twice, a0_in_a1, a0_outside, a0_repeated) == (3000, 0, 0, 0, 0, 0), (G, d)


@pytest.mark.parametrize("G", [G for G in GRIDS if admissible(G)])
def test_the_enumeration_tile_by_tile(program, G):
    """the same statement from the raw numbers, enumerated here: workgroup by workgroup from first, step and my_tiles"""
    for d in admissible(G):
        sizes = sorted({1, 2, d, d + 1, d + 2, G - 1, G, G + 1, 2 * (d + 1) + 1, 3 * (d + 1) + 1, G + G // d, G + G // d + 1, 1000, 2343, 2344, 39062} - {0})
        out = run(program, [[1, G, d, ntiles] for ntiles in sizes])
        for i, ntiles in enumerate(sizes):
            block = out[i * (G + 1):(i + 1) * (G + 1)]
            got_d, got_G, a0_first, a0_stride, a0_tiles, a1_tiles, b_step = block[0]
            assert (got_d, got_G, b_step) == (d, G, G + G // d)
            a1 = [r * (d + 1) for r in range(a1_tiles)]
            assert a1 == list(range(0, ntiles, d + 1)), (G, d, ntiles)
            b = []
            for u, (first, mine) in enumerate(block[1:]):
                assert first == u + 1 + u // d
                tiles = [first + j * b_step for j in range(mine)]
                assert all(t < ntiles for t in tiles) and (first + mine * b_step >= ntiles), (G, d, ntiles, u)
                b += tiles
            assert sorted(a1 + b) == list(range(ntiles)), (G, d, ntiles)
            a0 = [a0_first + u * a0_stride for u in range(a0_tiles)]
            assert len(set(a0)) == len(a0) and all(0 < t < ntiles and t % (d + 1) for t in a0), (G, d, ntiles)
            g = min(p for p in range(2, d + 2) if (d + 1) % p == 0)   # tiles 1, 1 + g, 1 + 2g, ... are all it may choose from
            assert a0_stride % g == 0 and a0_tiles == (0 if ntiles < 2 else min(G, (ntiles - 2) // g + 1)), (G, d, ntiles)
            if ntiles >= 2 * G * (d + 1):   # a large corpus: one full round, spread over (almost) all of it
                assert a0_tiles == G and a0[-1] >= ntiles - 1 - a0_stride - (d + 1) * G, (G, d, ntiles, a0[-1])


def test_the_rule_never_picks_a_d_that_does_not_divide_the_grid(program):
    cases = [(G, want) for G in (*GRIDS, 8, 96, 120, 128, 228, 240, 1024) for want in range(D_MIN, D_MAX + 1)]
    got = run(program, [[3, G, want] for G, want in cases])
    for (G, want), (d,) in zip(cases, got, strict=True):
        if not admissible(G):
            assert d == 0, (G, want)
        else:
            assert d in admissible(G) and abs(d - want) == min(abs(a - want) for a in admissible(G)), (G, want, d)


def plan_all(program, mode=1, want=32, min_rounds=3, G=256, ntiles=39062, k=10, ts_today=1536, family=TILE, ts=STATIC, res=0, sample_tiles=4096):
    """(on, d, a0_tiles, a0_stride)"""
    ((on, d, a0_tiles, a0_stride),) = run(program, [[4, mode, want, min_rounds, G, ntiles, k, ts_today, family, ts, res, sample_tiles]])
    return on, d, a0_tiles, a0_stride


def plan(program, **kw):
    return plan_all(program, **kw)[:2]


def test_when_the_cascade_applies(program):
    assert plan(program) == (1, 32)
    assert plan(program, want=16) == (1, 16) and plan(program, want=64) == (1, 64) and plan(program, want=40) == (1, 32)
    assert plan(program, mode=0) == (0, 0)
    # the size rule of mode 1: today's sample must have min_rounds rounds of workgroups; mode 2 does not ask
    assert plan(program, ntiles=4883, ts_today=512) == (0, 0)           # a 1.25M-row shard: two rounds
    assert plan(program, mode=2, ntiles=4883, ts_today=512) == (1, 32)
    assert plan(program, ts_today=3 * 256 - 1) == (0, 0) and plan(program, ts_today=3 * 256) == (1, 32)
    # only the static int8 tile program, staged
    for family, ts, res in ((0, 0, 0), (2, 3, 0), (TILE, 2, 0), (TILE, 1, 0), (TILE, 0, 0), (TILE, 1, 1)):
        assert plan(program, mode=2, family=family, ts=ts, res=res) == (0, 0), (family, ts, res)
    # a grid without a divisor in [16, 64]; a corpus of one tile; a first sample of fewer than 2k tiles
    assert plan(program, mode=2, G=7) == (0, 0) and plan(program, mode=2, G=1) == (0, 0)
    assert plan(program, mode=2, G=304) == (1, 38) and plan(program, mode=2, G=304, want=16) == (1, 16)
    assert plan(program, mode=2, ntiles=1) == (0, 0)
    assert plan(program, mode=2, ntiles=100, k=10) == (1, 32)            # 33 tiles 1, 4, 7, ... >= 20
    assert plan(program, mode=2, ntiles=100, k=17) == (0, 0)             # ... < 34
    assert plan(program, mode=2, ntiles=257, k=64) == (0, 0) and plan(program, mode=2, ntiles=2344, k=64) == (1, 32)


def test_the_first_sample_obeys_sample_tiles(program):
    """the sample's key buffer holds "sample_tiles" tiles per query (1 .. 65536): A0 takes no more, like the plain sample, and a value
    too small for 2k tiles switches the cascade off instead of overrunning the buffer"""
    assert plan_all(program, mode=2)[:3] == (1, 32, 256)
    for sample_tiles in (1, 19, 20, 64, 128, 255, 256, 257, 4096, 65536):
        on, d, a0_tiles, a0_stride = plan_all(program, mode=2, sample_tiles=sample_tiles)
        assert a0_tiles <= sample_tiles and a0_tiles <= 256, (sample_tiles, a0_tiles)
        assert on == int(min(sample_tiles, 256) >= 20), (sample_tiles, on)
        if on:
            assert a0_tiles == min(sample_tiles, 256) and a0_stride % 3 == 0 and 1 + (a0_tiles - 1) * a0_stride < 39062
    # ... with every admissible d and grid
    for G in (64, 256, 304):
        for d in admissible(G):
            for sample_tiles in (24, 100):
                on, got_d, a0_tiles, a0_stride = plan_all(program, mode=2, G=G, want=d, k=10, sample_tiles=sample_tiles)
                assert (on, got_d) == (1, d) and a0_tiles == min(sample_tiles, G), (G, d, sample_tiles, a0_tiles)
                tiles = [1 + u * a0_stride for u in range(a0_tiles)]
                assert all(t % (d + 1) and t < 39062 for t in tiles)
