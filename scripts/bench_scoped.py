#!/usr/bin/env python3
"""Namespace-scoped search against its two alternatives, on one GPU in one process.

    python scripts/bench_scoped.py [--rows 10000000 --dim 768 --dtype f32 --scopes 1000] --out profiles/scoped/bench_scoped.jsonl

One index of `rows` random unit rows is labelled three times: `scopes` equal scopes in contiguous runs (how the indexer job
writes a namespace), the same scopes round-robin (row % scopes: the worst locality), and one scope holding 10 % of the rows.
Points: B = 1; B = 32 in one scope; B = 256 spread over 256 scopes; B = 256 in one scope.  Per point, alternating in the timed loop:
  (a) scoped      codd_knn_search_scoped
  (b) whole       codd_knn_search with the same B on the whole index (no isolation: the code as it was before scopes existed)
  (c) own_index   codd_knn_search on a second index that holds only that scope's rows (a collection per namespace; one-scope points)
Times are host clock around a call that ends in a device synchronise, p50 of --reps after --warmup.  The scan's own time comes
from the engine's HIP-event log ("profile" option) in a separate loop; its bytes are rows read x row bytes, where a scope's rows
are read once per group of up to four of its queries.  One JSON line per point.
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
    p.add_argument("--scopes", type=int, default=1000)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoped", "bench_scoped.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_scoped.py measures on the GPU only"
    dev = "cuda:0"
    commit = head_commit(a.commit)
    n, ns = a.rows, a.scopes

    def chunk(c0):
        g = torch.Generator(device=dev).manual_seed(1000 + c0 // CHUNK)
        return torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev)

    ix = DeviceKnnIndex(a.dim, a.dtype, dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        ix.upsert_device(c0, chunk(c0))
    torch.cuda.synchronize()

    def own_index(members):
        """A second index with only these rows (sorted slots), regenerated from the seeds."""
        own = DeviceKnnIndex(a.dim, a.dtype, dev)
        own.reserve(len(members))
        at = 0
        for c0 in range(0, n, CHUNK):
            sel = members[(members >= c0) & (members < c0 + CHUNK)] - c0
            if sel.size:
                own.upsert_device(at, chunk(c0)[torch.from_numpy(sel).to(dev)].contiguous())
                at += sel.size
        torch.cuda.synchronize()
        return own

    gq = torch.Generator(device=dev).manual_seed(77)
    queries = torch.randn((256, a.dim), generator=gq, device=dev)
    row_bytes = ix.padded_dim * (4 if a.dtype == "f32" else 2)
    slots = np.arange(n, dtype=np.int64)
    per = -(-n // ns)
    layouts = [
        ("contiguous", (slots // per + 1).astype(np.uint32), True),
        ("round_robin", (slots % ns + 1).astype(np.uint32), True),
        ("ten_percent", np.where(slots < n // 10, 1, 2 + slots % (ns - 1)).astype(np.uint32), False),
    ]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for layout, labels, spread_point in layouts:
            t0 = time.perf_counter()
            ix.set_scopes(slots, labels)
            t_set = time.perf_counter() - t0
            builds0 = ix.stat("scope_builds")
            t_first = timed(lambda: ix.search_scoped_tensors(queries[:1], torch.ones(1, dtype=torch.int32, device=dev), a.k))
            assert ix.stat("scope_builds") == builds0 + 1
            sizes = np.bincount(labels, minlength=int(labels.max()) + 1)
            one = 1 if not spread_point else ns // 2          # the scope the one-scope points search
            own = own_index(np.flatnonzero(labels == one))
            points = [("B1", 1, [one]), ("B32_one_scope", 32, [one] * 32), ("B256_one_scope", 256, [one] * 256)]
            if spread_point:
                points.insert(2, ("B256_over_256_scopes", 256, list(range(1, 257))))
            for name, B, scopes in points:
                q = queries[:B].contiguous()
                s = torch.tensor(scopes, dtype=torch.int32, device=dev)
                one_scope = len(set(scopes)) == 1
                calls = {"scoped": lambda: ix.search_scoped_tensors(q, s, a.k), "whole": lambda: ix.search_tensors(q, a.k)}
                if one_scope:
                    calls["own_index"] = lambda: own.search_tensors(q, a.k)
                for _ in range(a.warmup):
                    for fn in calls.values():
                        timed(fn)
                ms = {key: [] for key in calls}
                for _ in range(a.reps):                        # alternating, so that a noisy neighbour hits all three alike
                    for key, fn in calls.items():
                        ms[key].append(timed(fn))
                # the scan kernel alone, from the engine's event log, in a loop of its own
                ix.set_option("profile", a.reps)
                for _ in range(a.reps):
                    calls["scoped"]()
                torch.cuda.synchronize()
                scan_ns, scan_ev = ix.stat("time_ns:scan"), ix.stat("events:scan")
                ix.set_option("profile", 0)
                groups = {}
                for sc in scopes:
                    groups[sc] = groups.get(sc, 0) + 1
                rows_read = sum(-(-cnt // QUERIES_PER_ITEM) * int(sizes[sc]) for sc, cnt in groups.items())
                scan_ms = scan_ns / 1e6 / max(scan_ev, 1)
                line = {
                    "commit": commit, "layout": layout, "point": name, "B": B, "k": a.k, "rows": n, "dim": a.dim, "dtype": a.dtype,
                    "scopes": int(labels.max()), "rows_in_scope": int(sizes[one]) if one_scope else int(sizes[1]),
                    "scoped_ms_p50": statistics.median(ms["scoped"]), "scoped_ms_min": min(ms["scoped"]),
                    "whole_index_ms_p50": statistics.median(ms["whole"]), "whole_index_ms_min": min(ms["whole"]),
                    "own_index_ms_p50": statistics.median(ms["own_index"]) if one_scope else None,
                    "speedup_vs_whole_index": statistics.median(ms["whole"]) / statistics.median(ms["scoped"]),
                    "ratio_to_own_index": statistics.median(ms["scoped"]) / statistics.median(ms["own_index"]) if one_scope else None,
                    "scan_kernel_ms": scan_ms, "scan_rows_read": rows_read, "scan_bytes": rows_read * row_bytes,
                    "scan_fraction_of_hbm_peak": rows_read * row_bytes / (scan_ms * 1e-3) / HBM_PEAK if scan_ms > 0 else None,
                    "set_scopes_s": t_set, "first_search_with_list_build_ms": t_first, "warmup": a.warmup, "reps": a.reps,
                }
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps(line))
            own.close()
    ix.close()


if __name__ == "__main__":
    main()
