#!/usr/bin/env python3
"""The exact scan under ChromaDB's three spaces, on one GPU in one process.

    python scripts/bench_spaces.py [--rows 10000000 --dim 768 --dtype f32] --out profiles/spaces/bench_spaces.jsonl

One corpus — bench.py's seeded randn rows (chunk c of 250,000 rows from seed 1234 + c), queries from seed 4321 — is stored four
times: an l2 index and an ip index (rows as given), and two cosine indexes (rows normalised) with "filter" = 0, so that every
batch of all four takes the exact scan and reads the same number of bytes.  The second cosine index is the yardstick's own
spread: the same code on the same box in the same loop.  Per B in {1, 8, 256} the four legs alternate in the timed loop.
  wall_ms        host clock around a search that ends in a device synchronise, p50 and min of --reps after --warmup
  scan_launch_ms the scan launch alone, from the engine's HIP-event log ("profile" option), in a loop of its own per leg, the
                 legs alternating per repetition; one launch serves the whole batch, ceil(B / 8) passes over the rows
  scan_bytes     passes x rows x row bytes; fraction_of_hbm_peak = scan_bytes / scan_launch time / 8 TB/s
One JSON line per (B, leg).  Measures on the GPU only.

    python scripts/bench_spaces.py --space-filter [--batches 16,64,256,512] --out profiles/space_filter/bench_space_filter.jsonl

The opt-in int8 filter leg of the two spaces against the scan it replaces: an l2 and an ip index, each searched
with "space_filter" on and off in the same loop (the same index, the option flipped per call), and a cosine index with "i8v2" = 0 —
the first-generation int8 GEMM, the like-for-like kernel.  Per (B, leg): wall time per batch (p50, min), and from the device
counters the hits and the survivors per query of the timed searches.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
CHUNK = 250_000
LEGS = [("l2", "l2"), ("ip", "ip"), ("cosine_a", "cosine"), ("cosine_b", "cosine")]


def head_commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--dtype", default="f32")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--batches", default="1,8,256")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--space-filter", action="store_true", help="measure the int8 filter leg of l2 and ip against the scan (DESIGN.md §21)")
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "spaces", "bench_spaces.jsonl"))
    a = p.parse_args()
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_spaces.py measures on the GPU only"
    dev = "cuda:0"
    commit = head_commit(a.commit)
    n = a.rows

    if a.space_filter:
        return space_filter_bench(a, torch, DeviceKnnIndex, dev, commit)

    indexes = {}
    for leg, space in LEGS:
        ix = DeviceKnnIndex(a.dim, a.dtype, dev, space=space)
        ix.reserve(n)
        for c0 in range(0, n, CHUNK):
            g = torch.Generator(device=dev).manual_seed(1234 + c0 // CHUNK)
            ix.upsert_device(c0, torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev), normalize=space == "cosine")
        if space == "cosine":
            ix.set_option("filter", 0)
        indexes[leg] = ix
    torch.cuda.synchronize()
    row_bytes = indexes["l2"].padded_dim * (4 if a.dtype == "f32" else 2)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for B in [int(b) for b in a.batches.split(",")]:
            q = torch.randn((B, a.dim), generator=torch.Generator(device=dev).manual_seed(4321), device=dev)
            calls = {leg: (lambda ix=ix: ix.search_tensors(q, a.k)) for leg, ix in indexes.items()}
            for _ in range(a.warmup):
                for fn in calls.values():
                    timed(fn)
            wall = {leg: [] for leg in calls}
            for _ in range(a.reps):                            # alternating, so that a noisy neighbour hits every leg alike
                for leg, fn in calls.items():
                    wall[leg].append(timed(fn))
            for ix in indexes.values():
                ix.set_option("profile", a.reps)
            for _ in range(a.reps):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            passes = -(-B // 8)
            scan_bytes = passes * n * row_bytes
            for leg, space in LEGS:
                ix = indexes[leg]
                scan_ns, scan_ev = ix.stat("time_ns:scan"), ix.stat("events:scan")
                ix.set_option("profile", 0)
                assert ix.stat("filter_passes") == 0 and scan_ev == a.reps, (leg, scan_ev)
                scan_ms = scan_ns / 1e6 / scan_ev
                line = {
                    "commit": commit, "leg": leg, "space": space, "B": B, "k": a.k, "rows": n, "dim": a.dim, "dtype": a.dtype,
                    "wall_ms_p50": statistics.median(wall[leg]), "wall_ms_min": min(wall[leg]),
                    "scan_launch_ms": scan_ms, "passes_over_the_rows": passes, "scan_ms_per_pass": scan_ms / passes,
                    "scan_group": ix.stat("last_scan_group"), "scan_bytes": scan_bytes,
                    "fraction_of_hbm_peak": scan_bytes / (scan_ms * 1e-3) / HBM_PEAK, "warmup": a.warmup, "reps": a.reps,
                }
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps(line))
    for ix in indexes.values():
        ix.close()


def space_filter_bench(a, torch, DeviceKnnIndex, dev, commit):
    n = a.rows
    indexes = {}
    for space in ("l2", "ip", "cosine"):
        ix = DeviceKnnIndex(a.dim, a.dtype, dev, space=space)
        ix.reserve(n)
        for c0 in range(0, n, CHUNK):
            g = torch.Generator(device=dev).manual_seed(1234 + c0 // CHUNK)
            ix.upsert_device(c0, torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev), normalize=space == "cosine")
        if space == "cosine":
            ix.set_option("i8v2", 0)
        indexes[space] = ix
    torch.cuda.synchronize()
    legs = [("l2_on", "l2", 1), ("l2_off", "l2", 0), ("ip_on", "ip", 1), ("ip_off", "ip", 0), ("cosine_i8", "cosine", None)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for B in [int(b) for b in a.batches.split(",")]:
            q = torch.randn((B, a.dim), generator=torch.Generator(device=dev).manual_seed(4321), device=dev)

            def call(space, on):
                ix = indexes[space]
                if on is not None:
                    ix.set_option("space_filter", on)
                ix.search_tensors(q, a.k)

            for _ in range(a.warmup):
                for _leg, space, on in legs:
                    timed(lambda: call(space, on))
            wall = {leg: [] for leg, _, _ in legs}
            counts = {leg: [0, 0, 0] for leg, _, _ in legs}
            keys = ("filter_hits", "filter_survivors", "filter_passes")
            for _ in range(a.reps):                            # alternating, so that a noisy neighbour hits every leg alike
                for leg, space, on in legs:
                    before = [indexes[space].stat(key) for key in keys]
                    wall[leg].append(timed(lambda: call(space, on)))
                    counts[leg] = [c + indexes[space].stat(key) - b for c, key, b in zip(counts[leg], keys, before)]
            for leg, space, on in legs:
                hits, surv, passes = counts[leg]
                line = {
                    "commit": commit, "leg": leg, "space": space, "space_filter": on, "B": B, "k": a.k, "rows": n, "dim": a.dim, "dtype": a.dtype,
                    "wall_ms_p50": statistics.median(wall[leg]), "wall_ms_min": min(wall[leg]), "filter_passes_per_search": passes / a.reps,
                    "hits_per_query": hits / (a.reps * B), "survivors_per_query": surv / (a.reps * B), "warmup": a.warmup, "reps": a.reps,
                }
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps(line))
    for ix in indexes.values():
        ix.close()


if __name__ == "__main__":
    main()
