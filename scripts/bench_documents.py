#!/usr/bin/env python3
"""`where_document` on one GPU in one process: the match kernel alone, the whole filtered query, and the host
evaluation of the same filter — the only thing that exists without the kernel.

    python scripts/bench_documents.py [--rows 10000000 --dim 768] --out profiles/documents/bench_documents.jsonl

One index of `rows` random unit rows and one document per row in the store's own format (`description | Category: value | ...`,
semantic_store.py), built from a small vocabulary so that needles of known selectivity exist: a word planted in about 0.1 %, 1 %,
10 % and 50 % of the documents.  Per needle:
  match_ms_p50          codd_knn_match_documents alone (memset + doc_match_kernel), HIP events around the call, p50 of --reps
  arena share of peak   arena bytes / that time, over 8 TB/s
  query cold / cached   Collection-level path — match_documents + search_masked_dev (cold), search_masked_dev on the cached words
                        (cached) — host clock around a call that ends in a device synchronise, B = 1 and B = 256
  host_eval_ms          `needle in doc` over the same documents (one pass; --host-reps passes, the median)
Two needles nobody planted stand for what users send: "e" (in every document, at a sizeable share of all positions) and " | "
(in every document, twice or more): the kernel's worst case, many matches per document.
The one-time snapshot build and upload (DeviceKnnIndex.set_documents: join, offsets, the engine's arena, the copy) is its own line.
Last, the whole `Collection.query(where_document=)` — grammar, caches, the engine calls, the numpy answer and the result lists — on a
collection of --collection-rows records (ids, metadata and documents as Python objects: the size a Collection holds comfortably),
cold (the needle's bitmap dropped before each call) and cached, B = 1 and B = 256, beside the host path forced on the same
collection (`needle in doc` and search_masked).
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
SHARES = (("rare", 0.001), ("few", 0.01), ("tenth", 0.1), ("half", 0.5))
NOUNS = ["request", "query", "connection", "queue", "cache", "disk", "memory", "thread", "packet", "session", "batch", "job"]
WHAT = ["duration", "count", "size", "throughput", "utilisation", "backlog", "failures", "retries"]
CATEGORIES = ["network", "database", "application", "storage", "runtime"]
SIGNALS = ["latency", "traffic", "errors", "saturation"]


def head_commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def make_documents(n, rng):
    """n documents in the store's format; marker words (zq<name>) planted with the shares of SHARES, independently."""
    u = {name: rng.random(n) < share for name, share in SHARES}
    a, b, c, s, num = (rng.integers(0, len(v), n) for v in (NOUNS, WHAT, CATEGORIES, SIGNALS, [0] * 1000))
    docs = []
    for i in range(n):
        marks = "".join(f" zq{name}" for name in u if u[name][i])
        docs.append(f"{NOUNS[a[i]].capitalize()} {WHAT[b[i]]} of service {num[i]}{marks} | Category: {CATEGORIES[c[i]]} | Golden Signal: {SIGNALS[s[i]]}")
    return docs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--host-reps", type=int, default=3)
    p.add_argument("--collection-rows", type=int, default=1_000_000)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "documents", "bench_documents.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_documents.py measures on the GPU only"
    dev = "cuda:0"
    commit = head_commit(a.commit)
    n = a.rows
    ix = DeviceKnnIndex(a.dim, "f32", dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        g = torch.Generator(device=dev).manual_seed(1000 + c0 // CHUNK)
        ix.upsert_device(c0, torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev))
    torch.cuda.synchronize()
    queries = torch.randn((256, a.dim), generator=torch.Generator(device=dev).manual_seed(77), device=dev)
    docs = make_documents(n, np.random.default_rng(9))
    t0 = time.perf_counter()
    raw = [d.encode("utf-8") for d in docs]
    encode_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.set_documents(raw)
    upload_s = time.perf_counter() - t0
    arena = ix.stat("doc_bytes")
    common = {"commit": commit, "rows": n, "dim": a.dim, "k": a.k, "warmup": a.warmup, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({**common, "point": "snapshot", "documents": n, "mean_document_bytes": (arena - n) / n, "arena_bytes": arena,
          "doc_tile_bytes": ix.stat("doc_tile_bytes"), "encode_utf8_s": encode_s, "set_documents_s": upload_s})

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, share in SHARES + (("every_e", None), ("every_bar", None)):
        needle = {"every_e": "e", "every_bar": " | "}.get(name, f"zq{name}")
        nb = needle.encode()
        host = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            mask = np.fromiter((needle in d for d in docs), dtype=bool, count=n)
            host.append((time.perf_counter() - t0) * 1e3)
        words = ix.match_documents(nb)
        got = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, mask), (needle, "the kernel and `needle in doc` disagree")
        ev = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ix.match_documents(nb)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ev.append(e0.elapsed_time(e1))
        match_ms = statistics.median(ev)
        line = {**common, "point": "needle", "needle": needle, "planted_share": share, "matched_documents": int(mask.sum()),
                "match_ms_p50": match_ms, "arena_bytes": arena, "arena_fraction_of_hbm_peak": arena / (match_ms * 1e-3) / HBM_PEAK,
                "host_eval_ms_p50": statistics.median(host)}
        for B in (1, 256):
            q = queries[:B].contiguous()
            cold = lambda: ix.search_masked_dev_tensors(q, ix.match_documents(nb), a.k)   # noqa: E731
            cached = lambda: ix.search_masked_dev_tensors(q, words, a.k)                  # noqa: E731
            for fn in (cold, cached):
                for _ in range(a.warmup):
                    timed(fn)
            line[f"query_cold_ms_p50_B{B}"] = statistics.median(timed(cold) for _ in range(a.reps))
            line[f"query_cached_ms_p50_B{B}"] = statistics.median(timed(cached) for _ in range(a.reps))
            line[f"whole_index_ms_p50_B{B}"] = statistics.median(timed(lambda: ix.search_tensors(q, a.k)) for _ in range(a.reps))
        emit(line)
    ix.close()

    # ---- the façade's whole call, at a size a Collection holds
    from codd_query_engine_amd import KnnClient

    m = min(a.collection_rows, n)
    col = KnnClient(device=dev).get_or_create_collection("bench")
    vec_rng = np.random.default_rng(3)
    for c0 in range(0, m, CHUNK):
        c1 = min(c0 + CHUNK, m)
        col.upsert(ids=[f"m{i}" for i in range(c0, c1)], embeddings=vec_rng.standard_normal((c1 - c0, a.dim)).astype(np.float32),
                   documents=docs[c0:c1])
    qh = queries.cpu().numpy()
    for name, share in SHARES:
        needle = f"zq{name}"
        wd = {"$contains": needle}
        line = {**common, "point": "collection_query", "collection_rows": m, "needle": needle, "planted_share": share}
        for B in (1, 256):
            def cold():
                col._doc_bits_cache.clear()
                col._doc_mask_cache.clear()
                return col.query(query_embeddings=qh[:B], n_results=a.k, where_document=wd, include=("distances",))

            def cached():
                return col.query(query_embeddings=qh[:B], n_results=a.k, where_document=wd, include=("distances",))

            device_answer = cached()
            for fn in (cold, cached):
                for _ in range(a.warmup):
                    timed(fn)
            line[f"query_cold_ms_p50_B{B}"] = statistics.median(timed(cold) for _ in range(a.reps))
            line[f"query_cached_ms_p50_B{B}"] = statistics.median(timed(cached) for _ in range(a.reps))
            # the host path on the same collection: what exists without the kernel
            col._has_device_documents = lambda: False
            try:
                host_answer = cold()
                line[f"host_path_cold_ms_p50_B{B}"] = statistics.median(timed(cold) for _ in range(a.host_reps))
                line[f"host_path_cached_ms_p50_B{B}"] = statistics.median(timed(cached) for _ in range(a.reps))
            finally:
                del col._has_device_documents
                col._doc_mask_cache.clear()
            assert host_answer["ids"] == device_answer["ids"], (needle, B, "the two paths disagree")
        emit(line)
    out.close()


if __name__ == "__main__":
    main()
