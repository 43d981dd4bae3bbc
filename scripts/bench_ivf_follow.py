#!/usr/bin/env python3
"""An IVF layout that follows writes on one GPU: the shard of scripts/bench_ivf.py (12.5M x 1024 fp16, 2,048 lists,
nprobe 8), k = 10.

    python scripts/bench_ivf_follow.py [--rows 12500000 --dim 1024 --nlist 2048 --nprobe 8] --out profiles/ivf_follow/bench_ivf_follow.jsonl

What it measures, host clock around a call that ends in a device synchronise, p10 / p50 / p90 of --reps:
  * a 1,000-row upsert_device with follow off (before the layout exists) and with follow on (rows become pending);
  * the IVF search at B = 1 and B = 256 in four settings: follow off, follow on with nothing pending — these two ALTERNATING in one
    loop (off, on, off again: the second off leg shows the run-to-run spread) —, follow on with 1,000 rows pending, and follow on
    with as many rows pending as the default threshold allows (one mean list);
  * recall@10 against the flat search with that many rows pending and after the fold;
  * one fold (codd_knn_ivf_refresh) against one build_ivf of the same index.
The one condition (exit status 1 when it does not hold): with follow on and nothing pending the search's p50 lies within the
spread of follow off — between the lowest p10 and the highest p90 of the two off legs of the same loop.
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

CHUNK = 250_000
NEVER = 1 << 32


def head_commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def summary(ms):
    s = sorted(ms)
    return {"p10_ms": s[len(s) // 10], "p50_ms": statistics.median(s), "p90_ms": s[(9 * len(s)) // 10], "n": len(s)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=12_500_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--centres", type=int, default=4096)
    p.add_argument("--nlist", type=int, default=2048)
    p.add_argument("--nprobe", type=int, default=8)
    p.add_argument("--iters", type=int, default=6)
    p.add_argument("--dtype", default="f16")
    p.add_argument("--noise", type=float, default=0.5)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--write-rows", type=int, default=1000)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_follow", "bench_ivf_follow.jsonl"))
    a = p.parse_args()
    import torch

    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_ivf_follow.py measures on the GPU only"
    dev = "cuda:0"
    n, k, w = a.rows, a.k, a.write_rows
    gc = torch.Generator(device=dev).manual_seed(7)
    centres = torch.nn.functional.normalize(torch.randn((a.centres, a.dim), generator=gc, device=dev), dim=1)

    def draw(m, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        which = torch.randint(0, a.centres, (m,), generator=g, device=dev)
        return centres[which] + a.noise * torch.randn((m, a.dim), generator=g, device=dev) / a.dim ** 0.5

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ix = DeviceKnnIndex(a.dim, a.dtype, dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        ix.upsert_device(c0, draw(min(CHUNK, n - c0), 100 + c0 // CHUNK).contiguous())
    torch.cuda.synchronize()

    common = {"commit": head_commit(a.commit), "rows": n, "dim": a.dim, "dtype": a.dtype, "nlist": a.nlist, "nprobe": a.nprobe, "k": k,
              "warmup": a.warmup, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    # the writes: fresh vectors for w-row ranges spread over the shard (every range is written with the same vectors each time)
    nwrites = 8
    starts = [int((i + 0.5) * n / nwrites) // 32 * 32 + 5 for i in range(nwrites)]
    fresh = [draw(w, 5000 + i).contiguous() for i in range(nwrites)]
    # 1. a w-row upsert_device with follow off: no layout yet, so nothing goes stale
    off_ms = [timed(lambda i=i: ix.upsert_device(starts[i], fresh[i])) for i in range(nwrites)]
    emit({**common, "point": "upsert_device", "follow": 0, "write_rows": w, **summary(off_ms[1:])})

    t0 = time.perf_counter()
    stats = ivf.build_ivf(ix, a.nlist, iters=a.iters)
    build_s = time.perf_counter() - t0
    emit({**common, "point": "index", "ivf_build_s": build_s, "ivf": stats})

    queries = draw(256, 9999)

    def search_legs(legs, B):
        """legs: name -> what to do before the search (set an option); alternating, one run of each per round"""
        q = queries[:B].contiguous()
        lat = {name: [] for name in legs}
        for i in range(a.warmup + a.reps):
            for name, before in legs.items():
                before()
                ms = timed(lambda: ivf.search_ivf(ix, q, k, a.nprobe))
                if i >= a.warmup:
                    lat[name].append(ms)
        return {name: summary(ms) for name, ms in lat.items()}

    def recall():
        _, truth = ix.search_tensors(queries, k)
        _, got = ivf.search_ivf(ix, queries, k, a.nprobe)
        return (got.unsqueeze(2) == truth.unsqueeze(1)).any(dim=2).float().mean().item()

    # 2. follow off against follow on with nothing pending, in one loop
    ok = True
    ix.set_option("ivf_fold_rows", NEVER)
    for B in (1, 256):
        legs = search_legs({"off_a": lambda: ix.set_option("ivf_follow", 0), "on_0_pending": lambda: ix.set_option("ivf_follow", 1),
                            "off_b": lambda: ix.set_option("ivf_follow", 0)}, B)
        lo = min(legs["off_a"]["p10_ms"], legs["off_b"]["p10_ms"])
        hi = max(legs["off_a"]["p90_ms"], legs["off_b"]["p90_ms"])
        within = lo <= legs["on_0_pending"]["p50_ms"] <= hi
        ok = ok and within
        emit({**common, "point": "search", "B": B, "pending": 0, "follow_off_a": legs["off_a"], "follow_on": legs["on_0_pending"], "follow_off_b": legs["off_b"],
              "off_spread_ms": [lo, hi], "on_p50_within_off_spread": within})
    assert ix.stat("ivf_delta_searches") == 0 and ix.stat("ivf_pending_rows") == 0

    # 3. follow on: w rows pending, then as many as the default threshold allows
    ix.set_option("ivf_follow", 1)
    threshold = -(-n // a.nlist)
    on_ms = [timed(lambda: ix.upsert_device(starts[0], fresh[0]))]
    assert ix.stat("ivf_pending_rows") == w
    for B in (1, 256):
        emit({**common, "point": "search", "B": B, "pending": w, "follow_on": search_legs({"on": lambda: None}, B)["on"]})
    i = 1
    while ix.stat("ivf_pending_rows") + w <= threshold and i < nwrites:
        on_ms.append(timed(lambda i=i: ix.upsert_device(starts[i], fresh[i])))
        i += 1
    rest = threshold - ix.stat("ivf_pending_rows")
    if rest > 0:
        ix.upsert_device(starts[0] + 2 * w, draw(rest, 6000).contiguous())
    emit({**common, "point": "upsert_device", "follow": 1, "write_rows": w, **summary(on_ms)})
    pending = ix.stat("ivf_pending_rows")
    for B in (1, 256):
        emit({**common, "point": "search", "B": B, "pending": pending, "default_threshold": threshold, "follow_on": search_legs({"on": lambda: None}, B)["on"]})
    recall_pending = recall()

    # 4. one fold against one build of the same index
    refreshes = ix.stat("ivf_refreshes")
    fold_ms = timed(ix.ivf_refresh)
    assert ix.stat("ivf_refreshes") == refreshes + 1 and ix.stat("ivf_pending_rows") == 0
    recall_folded = recall()
    for B in (1, 256):
        emit({**common, "point": "search", "B": B, "pending": 0, "after_fold": True, "follow_on": search_legs({"on": lambda: None}, B)["on"]})
    t0 = time.perf_counter()
    ivf.build_ivf(ix, a.nlist, iters=a.iters)
    rebuild_s = time.perf_counter() - t0
    emit({**common, "point": "fold", "folded_rows": pending, "fold_s": fold_ms / 1e3, "build_ivf_s": rebuild_s, "recall@10_pending": recall_pending,
          "recall@10_folded": recall_folded, "recall@10_rebuilt": recall()})
    out.close()
    ix.close()
    if not ok:
        print("bench_ivf_follow: follow on with nothing pending is OUTSIDE the spread of follow off", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
