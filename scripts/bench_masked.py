#!/usr/bin/env python3
"""Masked search, both routes, against the whole-index search, on one GPU in one process.

    python scripts/bench_masked.py [--rows 10000000 --dim 768 --dtype f32] --out profiles/masked/bench_masked.jsonl

One index of `rows` random unit rows.  Masks: 0.1 %, 1 %, 3 %, 10 % and 50 % of the rows at random, and one contiguous block of
10 % (rows [0, rows / 10): also labelled as a namespace, so that codd_knn_search_scoped answers the same question).  Batches of 1,
32 and 256 queries.  Per (mask, B) point, alternating in the timed loop:
  list / dense / auto   codd_knn_search_masked with "mask_route" 1 / 2 / 0
  whole                 codd_knn_search with the same B (no restriction)
  scoped                codd_knn_search_scoped on the block's namespace (the block mask only)
Times are host clock around a call that ends in a device synchronise, p50 of --reps after --warmup; they include the mask's way
to the device.  The heavy kernels' own time (scan, sample, filter, finalize) comes from the engine's HIP-event log ("profile"
option) in a loop of its own; `mask_upload_build_ms` is the call minus those: the host's pass over the words, the copy, the deny
launch or the list build, the small kernels.  The list route's bytes are ceil(B / 4) x m x row bytes.  One JSON line per point.
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
QUERIES_PER_ITEM = 4  # f32 / narrow rows (scope_nb in csrc/list_scan_kernels.h)


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
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--batches", default="1,32,256")
    p.add_argument("--mask-list-pct", type=int, default=None, help='the "mask_list_pct" option (default: the library\'s)')
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked", "bench_masked.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_masked.py measures on the GPU only"
    dev = "cuda:0"
    commit = head_commit(a.commit)
    n = a.rows
    ix = DeviceKnnIndex(a.dim, a.dtype, dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        g = torch.Generator(device=dev).manual_seed(1000 + c0 // CHUNK)
        ix.upsert_device(c0, torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev))
    torch.cuda.synchronize()
    slots = np.arange(n, dtype=np.int64)
    ix.set_scopes(slots, np.where(slots < n // 10, 1, 2).astype(np.uint32))
    if a.mask_list_pct is not None:
        ix.set_option("mask_list_pct", a.mask_list_pct)
    gq = torch.Generator(device=dev).manual_seed(77)
    queries = torch.randn((256, a.dim), generator=gq, device=dev)
    row_bytes = ix.padded_dim * (4 if a.dtype == "f32" else 2)
    rng = np.random.default_rng(5)
    masks = [(f"random_{share:g}", rng.random(n) < share) for share in (0.001, 0.01, 0.03, 0.1, 0.5)]
    masks.append(("block_0.1", slots < n // 10))

    def words_of(allow):
        padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
        padded[:n] = allow
        return np.packbits(padded, bitorder="little").view("<u4")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def kernels_ms(fn):
        """event-timed heavy kernels of one call (scan + sample + filter + finalize), mean over --reps"""
        ix.set_option("profile", 8 * a.reps)
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        total = sum(ix.stat(f"time_ns:{kind}") for kind in ("scan", "sample", "filter", "finalize"))
        ix.set_option("profile", 0)
        return total / 1e6 / a.reps

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for mask_name, allow in masks:
            words = words_of(allow)
            m = int(allow.sum())
            for B in [int(b) for b in a.batches.split(",")]:
                q = queries[:B].contiguous()

                def masked(route):
                    def call():
                        ix.set_option("mask_route", route)
                        return ix.search_masked_tensors(q, words, a.k)
                    return call

                calls = {"list": masked(1), "dense": masked(2), "auto": masked(0), "whole": lambda: ix.search_tensors(q, a.k)}
                if mask_name.startswith("block"):
                    s = torch.ones(B, dtype=torch.int32, device=dev)
                    calls["scoped"] = lambda: ix.search_scoped_tensors(q, s, a.k)
                same = [tuple(t.cpu().numpy().tobytes() for t in calls[key]()) for key in ("list", "dense", "auto")]
                assert same[0] == same[1] == same[2], (mask_name, B, "the routes disagree")
                for _ in range(a.warmup):
                    for fn in calls.values():
                        timed(fn)
                ms = {key: [] for key in calls}
                for _ in range(a.reps):                        # alternating, so that a noisy neighbour hits all alike
                    for key, fn in calls.items():
                        ms[key].append(timed(fn))
                p50 = {key: statistics.median(v) for key, v in ms.items()}
                lists0, dense0 = ix.stat("mask_list_searches"), ix.stat("mask_dense_searches")
                calls["auto"]()
                auto_route = "list" if ix.stat("mask_list_searches") > lists0 else "dense" if ix.stat("mask_dense_searches") > dense0 else "none"
                kern = {key: kernels_ms(calls[key]) for key in ("list", "dense", "whole")}
                h0, s0 = ix.stat("mask_filter_hits"), ix.stat("mask_filter_survivors")
                for _ in range(a.reps):
                    calls["dense"]()
                hits = (ix.stat("mask_filter_hits") - h0) / (a.reps * B)
                surv = (ix.stat("mask_filter_survivors") - s0) / (a.reps * B)
                list_bytes = -(-B // QUERIES_PER_ITEM) * m * row_bytes
                faster = "list" if p50["list"] <= p50["dense"] else "dense"
                line = {
                    "commit": commit, "mask": mask_name, "allowed_rows": m, "B": B, "k": a.k, "rows": n, "dim": a.dim, "dtype": a.dtype,
                    "list_ms_p50": p50["list"], "dense_ms_p50": p50["dense"], "auto_ms_p50": p50["auto"], "whole_index_ms_p50": p50["whole"],
                    "scoped_ms_p50": p50.get("scoped"), "auto_route": auto_route, "faster_route": faster,
                    "auto_miss_pct": 0.0 if auto_route == faster else 100.0 * (p50[auto_route] / p50[faster] - 1.0),
                    "list_kernels_ms": kern["list"], "dense_kernels_ms": kern["dense"], "whole_index_kernels_ms": kern["whole"],
                    "mask_upload_build_ms": {"list": p50["list"] - kern["list"], "dense": p50["dense"] - kern["dense"]},
                    "dense_hits_per_query": hits, "dense_survivors_per_query": surv,
                    "list_scan_bytes": list_bytes,
                    "list_scan_fraction_of_hbm_peak": list_bytes / (kern["list"] * 1e-3) / HBM_PEAK if kern["list"] > 0 else None,
                    "mask_list_pct": a.mask_list_pct, "warmup": a.warmup, "reps": a.reps,
                }
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps(line))
    ix.close()


if __name__ == "__main__":
    main()
