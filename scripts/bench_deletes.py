#!/usr/bin/env python3
"""What tombstones and compaction cost, on one GPU in one process.

    python scripts/bench_deletes.py [--rows 10000000 --dim 768 --dtype f32] --out profiles/deletes/bench_deletes.jsonl

One index of `rows` random unit rows.  Cases: (a) 1 % of the rows deleted at random, (b) one namespace of 10,000 contiguous rows
deleted, (c) 50 % deleted at random.  Per case, in this order on the SAME index (rebuilt between cases):
  search     step time at B = 1 and B = 256 before the delete and after it, p50 of --reps after --warmup (host clock around a call
             that ends in a device synchronise), with the filter_hits / filter_survivors the timed steps added per query
  compact    codd_knn_compact once: seconds, bytes moved (every row behind the first dead slot read once from its old place and
             written once to its new one; the two legs through the 64 MiB bounce buffer in between stay in cache and are not
             counted), the share of 8 TB/s that is, and the first search behind it (which rebuilds the shadows of the moved rows)
  rebuild    what a user had to do before compaction existed: a new index filled from the host with the live rows
             (codd_knn_upsert_host in pieces of 250,000 rows), timed once — the point of comparison
One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
CHUNK = 250_000


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--dtype", default="f32")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--cases", default="random_1pct,namespace_10k,random_50pct")
    p.add_argument("--no-rebuild", action="store_true", help="skip the rebuild-from-the-host comparison")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "deletes", "bench_deletes.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_deletes.py measures on the GPU only"
    dev = "cuda:0"
    n = a.rows
    row_bytes = ((a.dim + 63) // 64 * 64) * (4 if a.dtype == "f32" else 2)

    def chunk(c0):
        g = torch.Generator(device=dev).manual_seed(1000 + c0 // CHUNK)
        return torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev)

    def fill():
        ix = DeviceKnnIndex(a.dim, a.dtype, dev)
        ix.reserve(n)
        for c0 in range(0, n, CHUNK):
            ix.upsert_device(c0, chunk(c0))
        torch.cuda.synchronize()
        return ix

    gq = torch.Generator(device=dev).manual_seed(7)
    queries = {B: torch.randn((B, a.dim), generator=gq, device=dev) for B in (1, 256)}

    def timed(ix, B):
        q = queries[B]
        for _ in range(a.warmup):
            ix.search_tensors(q, a.k)
        torch.cuda.synchronize()
        h0, s0 = ix.stat("filter_hits"), ix.stat("filter_survivors")
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ix.search_tensors(q, a.k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        per = a.reps * B
        return {"p50_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
                "hits_per_query": (ix.stat("filter_hits") - h0) / per, "survivors_per_query": (ix.stat("filter_survivors") - s0) / per}

    def dead_slots(case):
        rng = np.random.default_rng(11)
        if case == "random_1pct":
            return np.sort(rng.permutation(n)[: n // 100])
        if case == "namespace_10k":
            first = n // 3
            return np.arange(first, first + min(10_000, n - first))
        if case == "random_50pct":
            return np.sort(rng.permutation(n)[: n // 2])
        raise SystemExit(f"unknown case {case}")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as out:
        for case in a.cases.split(","):
            ix = fill()
            rec = {"case": case, "rows": n, "dim": a.dim, "dtype": a.dtype, "k": a.k, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
            rec["before"] = {f"B{B}": timed(ix, B) for B in (1, 256)}
            dead = dead_slots(case)
            t0 = time.perf_counter()
            ix.delete(dead)
            rec["delete_s"] = time.perf_counter() - t0
            rec["dead_rows"] = int(ix.stat("dead_rows"))
            rec["tombstoned"] = {f"B{B}": timed(ix, B) for B in (1, 256)}
            # compaction: every live row from the first dead slot on leaves its old place and reaches its new one (HBM: one read, one write)
            live = n - dead.size
            moved_rows = live - int(dead[0])
            t0 = time.perf_counter()
            assert ix.compact() == live
            dt = time.perf_counter() - t0
            moved = 2 * moved_rows * row_bytes
            rec["compact"] = {"seconds": dt, "rows_moved": moved_rows, "bytes_moved": moved, "bytes_per_s": moved / dt, "share_of_8TBps": moved / dt / HBM_PEAK}
            t0 = time.perf_counter()
            ix.search_tensors(queries[256], a.k)
            torch.cuda.synchronize()
            rec["compact"]["first_search_ms"] = (time.perf_counter() - t0) * 1e3
            rec["compacted"] = {f"B{B}": timed(ix, B) for B in (1, 256)}
            if not a.no_rebuild:
                # the alternative: read the live rows out, build a new collection from the host
                host = np.empty((live, a.dim), dtype=np.float32)
                for c0 in range(0, live, CHUNK):
                    c = min(CHUNK, live - c0)
                    out_t = torch.empty((c, a.dim), dtype=torch.float32, device=dev)
                    from codd_query_engine_amd import native

                    native.check(native.load().codd_knn_copy_rows_f32(ix._h, c0, c, out_t.data_ptr(), ix._stream()), "codd_knn_copy_rows_f32")
                    host[c0 : c0 + c] = out_t.cpu().numpy()
                ix.close()
                t0 = time.perf_counter()
                fresh = DeviceKnnIndex(a.dim, a.dtype, dev)
                fresh.reserve(live)
                for c0 in range(0, live, CHUNK):
                    c = min(CHUNK, live - c0)
                    fresh.upsert(np.arange(c0, c0 + c, dtype=np.int64), host[c0 : c0 + c])
                torch.cuda.synchronize()
                rebuild = time.perf_counter() - t0
                t0 = time.perf_counter()
                fresh.search_tensors(queries[256], a.k)
                torch.cuda.synchronize()
                rec["rebuild_from_host"] = {"seconds": rebuild, "first_search_ms": (time.perf_counter() - t0) * 1e3, "ratio_to_compact": rebuild / dt}
                fresh.close()
                del host
            else:
                ix.close()
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
