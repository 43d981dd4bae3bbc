#!/usr/bin/env python3
"""IVF under ChromaDB's three spaces, on one GPU in one process.

    python scripts/bench_space_ivf.py [--rows 12500000 --dim 1024 --dtype f16 --nlist 2048] --out profiles/space_ivf/bench_space_ivf.jsonl

One clustered corpus (scripts/bench_ivf.py's, its unit centres scaled to norms uniform over --centre-norms, noise of norm --noise
around them) is stored
four times: an l2 and an ip index with "space_ivf" on (rows as given) and two cosine indexes (rows normalised); each gets its own
IVF layout from ivf.build_ivf (k-means in the index's own space).  The second cosine index is the yardstick's own spread: the same
code on the same box in the same loop.  Per B in --batches and nprobe in --nprobes the four legs alternate in the timed loop, then
each index's own flat search at the same B.
  event_ms   HIP events on the stream around one search (mean of --reps, the legs alternating)
  wall_ms    host clock around a search that ends in a device synchronise, p50 and min of --reps after --warmup
  recall@10  against the index's own flat search, over the B = max(--batches) queries
One JSON line per (leg, B, nprobe), nprobe 0 = the flat search; one line per leg for the build.  Measures on the GPU only.
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
    p.add_argument("--rows", type=int, default=12_500_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--dtype", default="f16")
    p.add_argument("--centres", type=int, default=4096)
    p.add_argument("--nlist", type=int, default=2048)
    p.add_argument("--iters", type=int, default=4)
    p.add_argument("--noise", type=float, default=0.5)
    p.add_argument("--centre-norms", default="0.5,2.0", help="the centres' norms are uniform over lo,hi (1,1: unit centres, as scripts/bench_ivf.py)")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--batches", default="1,256")
    p.add_argument("--nprobes", default="1,8,32")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "space_ivf", "bench_space_ivf.jsonl"))
    a = p.parse_args()
    import torch

    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_space_ivf.py measures on the GPU only"
    dev = "cuda:0"
    commit = head_commit(a.commit)
    n = a.rows
    gc = torch.Generator(device=dev).manual_seed(7)
    centres = torch.nn.functional.normalize(torch.randn((a.centres, a.dim), generator=gc, device=dev), dim=1)
    lo, hi = (float(x) for x in a.centre_norms.split(","))
    centres = centres * (lo + (hi - lo) * torch.rand((a.centres, 1), generator=gc, device=dev))

    def draw(m, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        which = torch.randint(0, a.centres, (m,), generator=g, device=dev)
        return (centres[which] + a.noise * torch.randn((m, a.dim), generator=g, device=dev) / a.dim ** 0.5).contiguous()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        line = {"commit": commit, "rows": n, "dim": a.dim, "dtype": a.dtype, "nlist": a.nlist, "k": a.k, "centres": a.centres, "centre_norms": a.centre_norms,
                "noise": a.noise, **line}
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    indexes = {}
    for leg, space in LEGS:
        ix = DeviceKnnIndex(a.dim, a.dtype, dev, space=space)
        ix.set_option("space_ivf", 1)
        ix.reserve(n)
        for c0 in range(0, n, CHUNK):
            ix.upsert_device(c0, draw(min(CHUNK, n - c0), 100 + c0 // CHUNK), normalize=space == "cosine")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = ivf.build_ivf(ix, a.nlist, iters=a.iters)
        emit({"leg": leg, "space": space, "what": "build", "build_s": time.perf_counter() - t0, "ivf": stats})
        indexes[leg] = ix

    batches = [int(b) for b in a.batches.split(",")]
    nprobes = [int(x) for x in a.nprobes.split(",")]
    qall = draw(max(batches), 9999)
    truth = {leg: ix.search_tensors(qall, a.k)[1] for leg, ix in indexes.items()}
    recall = {}
    for leg, ix in indexes.items():
        for nprobe in nprobes:
            got = ivf.search_ivf(ix, qall, a.k, nprobe)[1]
            recall[leg, nprobe] = (got.unsqueeze(2) == truth[leg].unsqueeze(1)).any(dim=2).float().mean().item()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def event(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for B in batches:
        q = qall[:B].contiguous()
        for nprobe in nprobes + [0]:
            if nprobe:
                calls = {leg: (lambda ix=ix: ivf.search_ivf(ix, q, a.k, nprobe)) for leg, ix in indexes.items()}
            else:
                calls = {leg: (lambda ix=ix: ix.search_tensors(q, a.k)) for leg, ix in indexes.items()}
            shared0 = {leg: ix.stat("ivf_shared_searches") for leg, ix in indexes.items()}
            for _ in range(a.warmup):
                for fn in calls.values():
                    wall(fn)
            w = {leg: [] for leg in calls}
            ev = {leg: [] for leg in calls}
            for _ in range(a.reps):                            # alternating, so that a noisy neighbour hits every leg alike
                for leg, fn in calls.items():
                    w[leg].append(wall(fn))
            for _ in range(a.reps):
                for leg, fn in calls.items():
                    ev[leg].append(event(fn))
            for leg, space in LEGS:
                emit({"leg": leg, "space": space, "what": "ivf" if nprobe else "flat", "B": B, "nprobe": nprobe,
                      "event_ms": statistics.mean(ev[leg]), "event_ms_min": min(ev[leg]), "wall_ms_p50": statistics.median(w[leg]), "wall_ms_min": min(w[leg]),
                      "recall@10": recall[leg, nprobe] if nprobe else 1.0, "recall_queries": max(batches),
                      "shared_scan": indexes[leg].stat("ivf_shared_searches") > shared0[leg], "warmup": a.warmup, "reps": a.reps})
    out.close()
    for ix in indexes.values():
        ix.close()


if __name__ == "__main__":
    main()
