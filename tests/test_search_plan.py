"""The route rules of a search (csrc/search_plan.h) without a device: tests/host/search_plan_main.cpp is compiled with the library's
own compiler used as a plain host compiler — the header takes no HIP — and fed cases on stdin.  What a filter pass runs for which
shape and options is the table of tests/_filter_stage_reference.py, which tests/test_gpu_filter_stages.py holds the device to."""

from __future__ import annotations

import itertools
import os
import re
import subprocess

import pytest

from codd_query_engine_amd import build
from tests import _filter_stage_reference as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, SPACE_FILTER, EXACT_SCAN, SMALL_BATCH, FILTER = range(5)
FAMILY = {"GEMM": 0, "TILE": 1, "TILE_F16": 2}
METRIC = {"cosine": 0, "ip": 1, "l2": 2}
DTYPE = {"f32": 0, "bf16": 1, "f16": 2}
CLAMPED = ("filter", "filter_min_rows", "filter_min_rows_small", "filter_min_batch")   # KNOBS: behind the table's rows
CLAMPED_DEFAULTS = {"filter": 1, "filter_min_rows": 1, "filter_min_rows_small": 100000, "filter_min_batch": 9}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_plan") / "search_plan_main")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", build.CSRC, "-I", build.INCLUDE,
           os.path.join(ROOT, "tests", "host", "search_plan_main.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "search_plan.h does not compile as plain C++17 without HIP:\n" + proc.stdout + proc.stderr
    return exe


def run(program, lines):
    """one output line per input line (the table command: one per row), each a list of integers"""
    proc = subprocess.run([program], input="".join(" ".join(str(int(v)) for v in line) + "\n" for line in lines), capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return [[int(v) for v in out.split()] for out in proc.stdout.splitlines()]


@pytest.fixture(scope="module")
def table(program):
    """the option table as the program prints it: name -> (default, lo, hi, rejected below, rejected above, stored lo, stored hi), in order"""
    proc = subprocess.run([program], input="0\n", capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    rows = [line.split() for line in proc.stdout.splitlines()]
    return {r[0]: tuple(int(v) for v in r[1:]) for r in rows}


def knobs(table, options=None):
    """KNOBS of a command line: the defaults with `options` (set_option names) over them"""
    options = dict(options or {})
    out = [options.pop(name, row[0]) for name, row in table.items()]
    out += [options.pop(name, CLAMPED_DEFAULTS[name]) for name in CLAMPED]
    assert not options, ("no such knob", options)
    return out


def shape(space, dtype, d, count, num_cus=256, all_normalized=None):
    return [METRIC[space], DTYPE[dtype], d, count, num_cus, int(space == "cosine" if all_normalized is None else all_normalized)]


def test_every_filter_stage_case_is_planned_as_the_device_runs_it(program, table):
    """the 56 (shape, options) -> program expectations that the device test pins, from plan_search and filter_program alone"""
    assert len(fs.CASES) == 56
    lines = []
    for case in fs.CASES:
        B = min(case.B, 256)   # (one pass, as in the device test: no case has more)
        lines.append([1, *knobs(table, {**fs.BASE_OPTIONS, **case.options}), *shape(case.space, case.dtype, case.d, case.rows(256)), B, fs.K, 0, 0, 0])
    for case, got in zip(fs.CASES, run(program, lines), strict=True):
        route, use8, can8, per_block, fused_prep, family, nbq, ts, res, el, sqd = got
        assert route == (FILTER if case.space == "cosine" else SPACE_FILTER), (case.id, route)
        assert use8 == case.el, case.id
        ran = {"family": family, "nbq": nbq, "ts": ts, "res": res, "el": el, "sqd": sqd}
        assert ran == {**case.program(), "family": FAMILY[case.family]}, (case.id, ran)
        if case.space == "cosine":
            assert can8 == int(case.options.get("shadow8", 1)) and fused_prep == 1, case.id
            if case.el:   # an int8 pass that runs the tile program has its bound per 32-row block
                assert per_block == int(case.family == "TILE"), case.id


def test_sample_tile_count_is_the_reference_geometry(program, table):
    grid = list(itertools.product((1, 20, 21, 255, 256, 511, 512, 513, 4096, 48829, 200000), (1, 10, 16, 17, 64, 128), (0, 1), (1, 2, 4, 8), (8, 256)))
    got = run(program, [[2, *knobs(table), *g] for g in grid])
    for (ntiles, k, use8, nbq, cus), (ts,) in zip(grid, got, strict=True):
        assert ts == fs.sample_geometry(ntiles, k, bool(use8), nbq, cus)[0], (ntiles, k, use8, nbq, cus, ts)


def test_per_block_derived_from_the_program_is_the_expression_it_replaced(program):
    """i8v2 x i8v2_half x resident_q x 1..32 K-steps x 1..1024 queries, on a cosine index"""
    ((cases, disagreements),) = run(program, [[3]])
    assert cases == 3 * 2 * 2 * 32 * 1024 and disagreements == 0


# a FilterWatch line: pending surv fb q8 q16 q8_sent q16_sent cooldown_left stat_cooldowns cooldown_surv8 cooldown_useless_epoch
RESET, QUERIES, SENT, OBSERVE = 0, 1, 2, 3
W = ("pending", "surv", "fb", "q8", "q16", "q8_sent", "q16_sent", "cooldown_left", "stat_cooldowns", "cooldown_surv8", "cooldown_useless_epoch")


def watch(program, ops):
    return [dict(zip(W, out, strict=True)) for out in run(program, [[4, *op] for op in ops])]


def window(q8, q16, surv, fb, epoch):
    """q8 / q16 queries filtered, a look sent, and its counters (running totals) observed: the state after each of the three"""
    return [(QUERIES, q8, q16), (SENT,), (OBSERVE, surv, fb, epoch)]


def test_watch_starts_a_cooldown_on_crowded_int8_windows(program):
    # 10 int8 queries leave 50,000 survivors
    s = watch(program, [(RESET,), *window(10, 0, 50_000, 0, 7)])
    assert s[2]["pending"] == 1 and (s[2]["q8_sent"], s[2]["q16_sent"]) == (10, 0)
    assert (s[3]["cooldown_left"], s[3]["stat_cooldowns"], s[3]["cooldown_surv8"]) == (256, 1, 5000)
    assert s[3]["pending"] == 0 and (s[3]["surv"], s[3]["fb"]) == (50_000, 0)
    # 100 int8 queries, 6 of them sent to the fallback: a cooldown; 5: none
    six = watch(program, [(RESET,), *window(100, 0, 0, 6, 7)])[-1]
    five = watch(program, [(RESET,), *window(100, 0, 0, 5, 7)])[-1]
    assert (six["cooldown_left"], six["stat_cooldowns"]) == (256, 1)
    assert (five["cooldown_left"], five["stat_cooldowns"]) == (0, 0)


def test_watch_ends_a_cooldown_the_two_byte_filter_does_not_pay_for(program):
    start = [(RESET,), *window(10, 0, 50_000, 0, 7)]                       # a cooldown started at 5,000 survivors per query
    # a 2-byte-only window at 3,000 per query changes nothing ...
    s = watch(program, [*start, *window(0, 10, 80_000, 0, 7)])[-1]
    assert (s["cooldown_left"], s["cooldown_useless_epoch"], s["stat_cooldowns"]) == (256, -1, 1)
    # ... at 4,500 per query (above shadow8_max_surv and above half of 5,000) the cooldown ends and the epoch is remembered
    ended = [*start, *window(0, 10, 80_000, 0, 7), *window(0, 10, 125_000, 0, 7)]
    s = watch(program, ended)[-1]
    assert (s["cooldown_left"], s["cooldown_useless_epoch"], s["stat_cooldowns"]) == (0, 7, 1)
    # an int8 window over the limit at the same epoch starts no cooldown; at a later epoch it does
    same = watch(program, [*ended, *window(10, 0, 175_000, 0, 7)])[-1]
    assert (same["cooldown_left"], same["stat_cooldowns"]) == (0, 1)
    later = watch(program, [*ended, *window(10, 0, 175_000, 0, 8)])[-1]
    assert (later["cooldown_left"], later["stat_cooldowns"], later["cooldown_surv8"]) == (256, 2, 5000)


def test_watch_bookkeeping(program):
    # a mixed window only moves the baselines
    s = watch(program, [(RESET,), *window(10, 10, 1_000_000, 50, 7)])[-1]
    assert (s["cooldown_left"], s["stat_cooldowns"], s["cooldown_useless_epoch"]) == (0, 0, -1)
    assert (s["surv"], s["fb"], s["q8"], s["q16"]) == (1_000_000, 50, 0, 0)
    # the queries counted drop by what was sent, every time: those filtered while the copy was in flight stay
    for q8, q16 in ((10, 0), (0, 10), (10, 10)):
        s = watch(program, [(RESET,), (QUERIES, q8, q16), (SENT,), (QUERIES, 3, 4), (OBSERVE, 0, 0, 7)])
        assert (s[3]["q8"], s[3]["q16"], s[3]["q8_sent"], s[3]["q16_sent"]) == (q8 + 3, q16 + 4, q8, q16)
        assert (s[4]["q8"], s[4]["q16"]) == (3, 4)
    # a look is due after each of the first 32 searches, then after every 8th
    due = [d for (d,) in run(program, [[5, n] for n in range(1, 81)])]
    assert due == [int(n <= 32 or n % 8 == 0) for n in range(1, 81)]
    assert due[32 - 1] == 1 and due[33 - 1] == 0 and due[40 - 1] == 1


def test_mask_takes_dense(program, table):
    big = shape("cosine", "f32", 768, 1_000_000)
    tail = [256, 10]
    got = run(program, [[6, *knobs(table, {"mask_route": 1}), *big, *tail, 1_000_000],
                        [6, *knobs(table, {"mask_route": 2}), *big, *tail, 1],
                        [6, *knobs(table), *big, *tail, 1_000_000],
                        [6, *knobs(table), *big, *tail, 1]])
    assert [g[0] for g in got] == [0, 1, 1, 0]


def documented_defaults():
    """"name" (N...) of the option text in include/codd_knn.h"""
    with open(os.path.join(build.INCLUDE, "codd_knn.h"), encoding="utf-8") as f:
        text = re.sub(r"\n \*\s*", " ", f.read())
    text = text[text.index('options: "scan_blocks_per_cu"'):text.index('stats  : "searches"')]
    return {name: int(value) for name, value in re.findall(r'"(\w+)"\s*\((\d+)[:;,)]', text)}


def test_option_table(table):
    """every "integer in [lo, hi]" option: its default is the documented one, lo - 1 and hi + 1 are rejected and leave the knob alone,
    lo and hi are stored.  (No stat of an option's name can be read without a device; "space_filter", the one row that has such a
    stat, is held to its documented default like the others.)"""
    documented = documented_defaults()
    assert len(table) == 23
    for name, (default, lo, hi, below, above, at_lo, at_hi) in table.items():
        assert documented.get(name) == default, (name, default, documented.get(name))
        assert lo <= default <= hi, name
        assert (below, above, at_lo, at_hi) == (1, 1, 1, 1), name
