#!/usr/bin/env python
"""
What a `$regex` costs on one MI355X, on the corpus recipe of scripts/bench_documents.py: store-format documents with
marker words planted at known shares.

    python scripts/bench_regex.py [--rows 2000000] [--out profiles/regex/bench_regex.jsonl]

Per pattern — a rare one, a 10 % one, one every document matches, an anchored one that dies at the first byte and an anchored one
that matches some — one JSON line:
  dfa_ms_p50            codd_knn_match_documents_dfa alone (table upload + doc_regex_kernel), HIP events around the call, p50 of --reps
  arena_fraction_of_hbm_peak   arena bytes / that time, as a share of 8 TB/s
  literal_match_ms_p50  doc_match_kernel on the literal the pattern contains, the same way: the substring kernel on the same box
  host_eval_ms          one `re.search` pass over the same documents on the host (what a new pattern costs without the kernel)
  compile_ms            pattern -> byte DFA on the host
  query cold / cached   match_documents_dfa + search_masked_dev (cold), search_masked_dev on the cached words, B = 1
The kernel's bitmap is compared with the host pass bit for bit before anything is timed.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_documents import CHUNK, HBM_PEAK, head_commit, make_documents  # noqa: E402

PATTERNS = [
    ("rare", r"zqrare( |$)", "zqrare"),
    ("tenth", r"zq(tenth|nothing)", "zqtenth"),
    ("all", r"of service [0-9]+", "of service"),
    ("anchored_dies", r"^Zz.*latency$", "latency"),
    ("anchored_some", r"^(Request|Query) .*(latency|errors)$", "Request "),
]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=2_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "regex", "bench_regex.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd.knn_index import DeviceKnnIndex
    from codd_query_engine_amd.regex_dfa import compile_search_dfa

    assert torch.cuda.is_available(), "bench_regex.py measures on the GPU only"
    dev = "cuda:0"
    n = a.rows
    ix = DeviceKnnIndex(a.dim, "f32", dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        g = torch.Generator(device=dev).manual_seed(1000 + c0 // CHUNK)
        ix.upsert_device(c0, torch.randn((min(CHUNK, n - c0), a.dim), generator=g, device=dev))
    torch.cuda.synchronize()
    q = torch.randn((1, a.dim), generator=torch.Generator(device=dev).manual_seed(77), device=dev)
    docs = make_documents(n, np.random.default_rng(9))
    ix.set_documents([d.encode("utf-8") for d in docs])
    arena = ix.stat("doc_bytes")
    common = {"commit": head_commit(a.commit), "rows": n, "dim": a.dim, "k": a.k, "warmup": a.warmup, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({**common, "point": "snapshot", "documents": n, "mean_document_bytes": (arena - n) / n, "arena_bytes": arena,
          "doc_regex_tile_bytes": ix.stat("doc_regex_tile_bytes"), "doc_regex_run_docs": ix.stat("doc_regex_run_docs")})

    def events(fn):
        ev = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ev.append(e0.elapsed_time(e1))
        return statistics.median(ev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, pattern, literal in PATTERNS:
        t0 = time.perf_counter()
        dfa = compile_search_dfa(pattern, True)
        compile_ms = (time.perf_counter() - t0) * 1e3
        assert dfa is not None, pattern
        search = re.compile(pattern).search
        t0 = time.perf_counter()
        mask = np.fromiter((search(d) is not None for d in docs), dtype=bool, count=n)
        host_ms = (time.perf_counter() - t0) * 1e3
        words = ix.match_documents_dfa(dfa)
        got = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, mask), (pattern, "the kernel and re.search disagree")
        dfa_ms = events(lambda: ix.match_documents_dfa(dfa))
        lit = literal.encode()
        lit_ms = events(lambda: ix.match_documents(lit))
        cold = lambda: ix.search_masked_dev_tensors(q, ix.match_documents_dfa(dfa), a.k)   # noqa: E731
        cached = lambda: ix.search_masked_dev_tensors(q, words, a.k)                        # noqa: E731
        for fn in (cold, cached):
            for _ in range(a.warmup):
                timed(fn)
        emit({**common, "point": "pattern", "name": name, "pattern": pattern, "dfa_states": dfa.nstates, "dfa_classes": dfa.nclasses,
              "matched_documents": int(mask.sum()), "compile_ms": compile_ms, "dfa_ms_p50": dfa_ms, "arena_bytes": arena,
              "arena_fraction_of_hbm_peak": arena / (dfa_ms * 1e-3) / HBM_PEAK, "literal": literal, "literal_match_ms_p50": lit_ms,
              "host_eval_ms": host_ms, "query_cold_ms_p50_B1": statistics.median(timed(cold) for _ in range(a.reps)),
              "query_cached_ms_p50_B1": statistics.median(timed(cached) for _ in range(a.reps))})
    ix.close()


if __name__ == "__main__":
    main()
