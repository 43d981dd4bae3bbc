#!/usr/bin/env python3
"""Text -> vector on the host and on the device, one process on one GPU: where the device route starts to win.

    python scripts/bench_embed.py [--dim 768] --out profiles/embed/bench_embed.jsonl

Both routes end with the vectors in device memory, which is where the search wants them:
  host route    HashingEmbeddingFunction.__call__ (its token cache warm) and the upload of the [n, dim] matrix
  device route  HashingEmbeddingFunction.embed_on_device: packing the texts, codd_knn_embed_texts_host (staging, one copy, one kernel)
Host wall clock around a call that ends in a device synchronise.  The routes alternate in rounds on the same texts (--rounds rounds of
--reps calls each, per route); a point's figure is the median over all its calls, its SPREAD the distance between the highest and the
lowest round median of one route (the larger of the two routes').  The results are compared bit for bit before anything is timed.
  query   bench.py's query texts (3-12 words of its word list), batch sizes 1, 2, 4 ... 256
  ingest  10,000 documents of about 200 bytes in the store's format, one call
DEVICE_EMBED_MIN_TEXTS (knn_client.Collection) is the smallest batch size from which, at every size measured, the device route's
median stays below the host route's by more than the spread; the last line names it.  --kernel-only runs the device route alone,
for a profiler run of its own.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ["http", "request", "latency", "error", "rate", "cpu", "memory", "usage", "disk", "network", "queue", "depth", "database", "query",
         "duration", "seconds", "bytes", "total", "p99", "timeout", "connection", "pool", "gc", "pause", "heap", "cache", "hit", "ratio"]
CATEGORIES = ["network", "database", "application", "storage", "runtime"]
SIGNALS = ["latency", "traffic", "errors", "saturation"]


def head_commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def query_texts(n, seed=11):
    rnd = random.Random(seed)
    return [" ".join(rnd.choice(WORDS) for _ in range(rnd.randint(3, 12))) for _ in range(n)]


def ingest_documents(n, seed=12):
    rnd = random.Random(seed)
    docs = []
    for i in range(n):
        words = " ".join(rnd.choice(WORDS) for _ in range(rnd.randint(14, 22)))
        docs.append(f"{words.capitalize()} of service {i % 1000} | Category: {rnd.choice(CATEGORIES)} | Subcategory: http | Golden Signal: "
                    f"{rnd.choice(SIGNALS)} | Meter Type: gauge")
    return docs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=10, help="calls per round and route (rounds * reps >= 30)")
    p.add_argument("--ingest-rounds", type=int, default=3)
    p.add_argument("--ingest-reps", type=int, default=3)
    p.add_argument("--kernel-only", action="store_true")
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed", "bench_embed.jsonl"))
    a = p.parse_args()
    assert a.rounds * a.reps >= 30
    import numpy as np
    import torch

    from codd_query_engine_amd.embedding import HashingEmbeddingFunction

    assert torch.cuda.is_available(), "bench_embed.py measures on the GPU only"
    dev = "cuda:0"
    e = HashingEmbeddingFunction(a.dim)
    texts, docs = query_texts(256), ingest_documents(10_000)

    def host_route(batch):
        out = torch.from_numpy(e(batch)).to(dev)
        torch.cuda.synchronize()
        return out

    def device_route(batch):
        out = e.embed_on_device(batch, dev)
        torch.cuda.synchronize()
        return out

    if a.kernel_only:
        for _ in range(a.warmup + a.reps):
            for batch in (texts[:1], texts[:16], texts, docs):
                device_route(batch)
        e.close()
        return

    def timed(fn, batch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(batch)
        return (time.perf_counter() - t0) * 1e3

    def point(batch, rounds, reps):
        same = np.array_equal(host_route(batch).cpu().numpy().view(np.uint32), device_route(batch).cpu().numpy().view(np.uint32))
        assert same, "the two routes disagree"
        for fn in (host_route, device_route):
            for _ in range(a.warmup):
                fn(batch)
        runs = {"host": [], "device": []}
        for _ in range(rounds):
            for name, fn in (("host", host_route), ("device", device_route)):
                runs[name].append([timed(fn, batch) for _ in range(reps)])
        med = {name: statistics.median(t for r in rs for t in r) for name, rs in runs.items()}
        per_round = {name: [statistics.median(r) for r in rs] for name, rs in runs.items()}
        spread = max(max(m) - min(m) for m in per_round.values())
        return {"texts": len(batch), "text_bytes": sum(len(t) for t in batch), "host_route_ms_p50": med["host"], "device_route_ms_p50": med["device"],
                "spread_ms": spread, "host_round_medians_ms": per_round["host"], "device_round_medians_ms": per_round["device"],
                "device_wins": med["device"] < med["host"] - spread}

    common = {"commit": head_commit(a.commit), "dim": a.dim, "trigram_weight": e.trigram_weight, "warmup": a.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    sizes = [1 << i for i in range(9)]
    wins = {}
    for B in sizes:
        line = point(texts[:B], a.rounds, a.reps)
        wins[B] = line["device_wins"]
        emit({**common, "point": "query", "rounds": a.rounds, "reps": a.reps, **line})
    emit({**common, "point": "ingest", "rounds": a.ingest_rounds, "reps": a.ingest_reps, **point(docs, a.ingest_rounds, a.ingest_reps)})
    chosen = None
    for B in reversed(sizes):   # the smallest size from which every measured size is a win
        if not wins[B]:
            break
        chosen = B
    emit({**common, "point": "threshold", "device_embed_min_texts": chosen,
          "rule": "smallest measured batch size from which the device route's median is below the host route's by more than the spread, at every larger size too"})
    out.close()
    e.close()


if __name__ == "__main__":
    main()
