#!/usr/bin/env python3
"""A row mask under the coarse-IVF search on one GPU: the shard of scripts/bench_ivf.py (12.5M x 1024 fp16, 2,048
lists, nprobe 8), B = 1 and B = 256, k = 10.

    python scripts/bench_ivf_masked.py [--rows 12500000 --dim 1024 --nlist 2048 --nprobe 8] --out profiles/ivf_masked/bench_ivf_masked.jsonl

Masks: 0.01 %, 1 %, 10 % and 50 % of the rows at random, and one cached `$contains` bitmap (codd_knn_match_documents over one short
document per row; the needle planted in 10 % of them).  Per mask and batch size, ALTERNATING in one loop so that the three see the
same clocks: the masked IVF search (device words, codd_knn_ivf_search_masked_dev), the unmasked IVF search, and the flat
search_masked_dev under the same words; host clock around a call that ends in a device synchronise, p50 of --reps.
hits_of_k: how many of the k hits the mask leaves inside the probed lists, mean and minimum over the 256 queries — the masked IVF
search never probes further, so a small mask returns few hits (the flat masked search returns k of them).
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
    p.add_argument("--centres", type=int, default=4096)
    p.add_argument("--nlist", type=int, default=2048)
    p.add_argument("--nprobe", type=int, default=8)
    p.add_argument("--iters", type=int, default=6)
    p.add_argument("--dtype", default="f16")
    p.add_argument("--noise", type=float, default=0.5)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_masked", "bench_ivf_masked.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    from codd_query_engine_amd import ivf, native
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    assert torch.cuda.is_available(), "bench_ivf_masked.py measures on the GPU only"
    dev = "cuda:0"
    n, k = a.rows, a.k
    gc = torch.Generator(device=dev).manual_seed(7)
    centres = torch.nn.functional.normalize(torch.randn((a.centres, a.dim), generator=gc, device=dev), dim=1)

    def draw(m, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        which = torch.randint(0, a.centres, (m,), generator=g, device=dev)
        return centres[which] + a.noise * torch.randn((m, a.dim), generator=g, device=dev) / a.dim ** 0.5

    ix = DeviceKnnIndex(a.dim, a.dtype, dev)
    ix.reserve(n)
    for c0 in range(0, n, CHUNK):
        ix.upsert_device(c0, draw(min(CHUNK, n - c0), 100 + c0 // CHUNK).contiguous())
    torch.cuda.synchronize()

    # one short document per row, the needle planted in 10 % of them; straight through the C ABI (no Python list of 12.5M objects)
    rng = np.random.default_rng(9)
    plain, marked = np.frombuffer(b"queue backlog of service", dtype=np.uint8), np.frombuffer(b"queue backlog of service zqtenth", dtype=np.uint8)
    has = rng.random(n) < 0.10
    lengths = np.where(has, marked.shape[0], plain.shape[0]).astype(np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    wide = np.broadcast_to(marked, (n, marked.shape[0]))
    blob = np.ascontiguousarray(wide[np.arange(marked.shape[0])[None, :] < lengths[:, None]])
    native.check(native.load().codd_knn_set_documents_host(ix._h, blob.ctypes.data, offsets.ctypes.data, n), "codd_knn_set_documents_host")
    del wide, blob
    t0 = time.perf_counter()
    stats = ivf.build_ivf(ix, a.nlist, iters=a.iters)     # (after the documents: an upsert would make them stale, a build does not)
    build_s = time.perf_counter() - t0

    nwords = (n + 31) // 32
    masks = {}
    # (0.01 %: about five allowed rows in eight lists of 6,100 — where the probed lists run out of allowed rows)
    for name, share in (("random_0.01pct", 0.0001), ("random_1pct", 0.01), ("random_10pct", 0.10), ("random_50pct", 0.50)):
        bits = rng.random(nwords * 32) < share
        bits[n:] = False
        masks[name] = torch.from_numpy(np.packbits(bits, bitorder="little").view("<u4").view(np.int32).copy()).to(dev)
    masks["contains_cached"] = ix.match_documents(b"zqtenth")
    assert ix.stat("docs_valid") == 1
    torch.cuda.synchronize()

    queries = draw(256, 9999)
    common = {"commit": head_commit(a.commit), "rows": n, "dim": a.dim, "dtype": a.dtype, "nlist": a.nlist, "nprobe": a.nprobe, "k": k,
              "warmup": a.warmup, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({**common, "point": "index", "ivf_build_s": build_s, "ivf": stats})

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, words in masks.items():
        allowed = int(np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n].sum())
        keys = ix.ivf_search_keys_masked_dev(queries, words, k, a.nprobe)
        hits = (keys != 0).sum(dim=1).float()
        flat_keys = ix.search_keys_masked_dev(queries, words, k)
        recall = ((keys.unsqueeze(2) == flat_keys.unsqueeze(1)) & (flat_keys != 0).unsqueeze(1)).any(dim=1).float().sum() / (flat_keys != 0).sum()
        line = {**common, "point": "mask", "mask": name, "allowed_rows": allowed, "allowed_share": allowed / n,
                "hits_of_k_mean": hits.mean().item(), "hits_of_k_min": int(hits.min().item()), "recall_vs_flat_masked": recall.item()}
        for B in (1, 256):
            q = queries[:B].contiguous()
            legs = {
                "ivf_masked_dev": lambda: ix.ivf_search_masked_dev_tensors(q, words, k, a.nprobe),
                "ivf_unmasked": lambda: ivf.search_ivf(ix, q, k, a.nprobe),
                "flat_masked_dev": lambda: ix.search_masked_dev_tensors(q, words, k),
            }
            lat = {leg: [] for leg in legs}
            for i in range(a.warmup + a.reps):
                for leg, fn in legs.items():       # alternating: one run of each per round
                    ms = timed(fn)
                    if i >= a.warmup:
                        lat[leg].append(ms)
            for leg in legs:
                line[f"{leg}_ms_p50_B{B}"] = statistics.median(lat[leg])
        emit(line)
    out.close()
    ix.close()


if __name__ == "__main__":
    main()
