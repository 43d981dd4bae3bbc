#!/usr/bin/env python
"""
What `where=` costs on the host route and on the device route, on one MI355X, in one process.

    python scripts/bench_where.py [--rows 1000000] [--out profiles/where/bench_where.jsonl]

Two collections over the same --rows x --dim f32 rows and the same metadata — one categorical key with 3 values ("cat3"), one with
1,000 ("cat1000"), one float key with all values distinct ("x") — one on the host route, one opted in (KnnClient(device_where=True)).
Per filter ($eq, $in of 8 values, $gt, a 4-leaf $and / $or) one JSON line, times in ms, B = 1:
  first_after_write_host / _device   the first filtered query after an upsert of 1,000 rows (median of --writes such writes): the host
                                     route rebuilds its per-key value index, the device route evaluates the program over its columns
  cached_host / _device              the same filter again
  eval_call_ms_p50                   one engine.eval_where(program) — the binding's work on the host, the enqueue and where_eval_kernel —
                                     between two HIP events, p50 of --reps: what a new filter's bitmap costs a caller, NOT the kernel alone
  eval_back_to_back_ms               codd_knn_eval_where called --burst times in a row on a prepared program and output buffer, two
                                     events around the burst, per launch: an upper bound of the kernel's time (the launch rate may be
                                     what bounds it), and
  back_to_back_fraction_of_hbm_peak  rows x 9 B x distinct columns over that time, as a share of 8 TB/s: a lower bound of the kernel's
  column_build_ms                    the one-off build of the columns the filter names (one pass over the records + one upload each)
  upsert_host / _device, encode_ms   the 1,000-row upsert itself on either collection (ids that exist: the rows are rewritten), and the
                                     column encoding alone inside the opted-in one (every column built so far)
  append_host / _device              the same upsert with 1,000 NEW ids: the count grows, and with it the mirrors of every column
The two routes' answers are compared (ids and distance bits) before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_documents import HBM_PEAK, head_commit  # noqa: E402

CHUNK = 100_000
WRITE_ROWS = 1_000


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--writes", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--burst", type=int, default=200)
    p.add_argument("--commit", default=None, help="git rev-parse HEAD of the tree (when the tree is a copy without .git)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "where", "bench_where.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch

    import ctypes

    from codd_query_engine_amd import KnnClient, native
    from codd_query_engine_amd import where_columns as wc

    assert torch.cuda.is_available(), "bench_where.py measures on the GPU only"
    n = a.rows
    rng = np.random.default_rng(5)
    x = rng.permutation(n) / n   # all distinct
    metadata = lambda i: {"cat3": "abc"[i % 3], "cat1000": f"v{(i * 7919) % 1000}", "x": float(x[i])}  # noqa: E731
    host = KnnClient().get_or_create_collection("host")
    device = KnnClient(device_where=True).get_or_create_collection("device")
    t0 = time.perf_counter()
    for c0 in range(0, n, CHUNK):
        c1 = min(n, c0 + CHUNK)
        vecs = np.random.default_rng(1000 + c0 // CHUNK).standard_normal((c1 - c0, a.dim)).astype(np.float32)
        ids, mds = [f"id{i}" for i in range(c0, c1)], [metadata(i) for i in range(c0, c1)]
        for col in (host, device):
            col.upsert(ids=ids, embeddings=vecs, metadatas=mds)
    setup_s = time.perf_counter() - t0
    q = np.random.default_rng(77).standard_normal((1, a.dim)).astype(np.float32)
    common = {"commit": head_commit(a.commit), "rows": n, "dim": a.dim, "k": a.k, "writes": a.writes, "reps": a.reps, "write_rows": WRITE_ROWS}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({**common, "point": "setup", "setup_s": setup_s})

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, result

    def events(fn):
        ev = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                ev.append(e0.elapsed_time(e1))
        return statistics.median(ev)

    ask = lambda col, where: col.query(query_embeddings=q, n_results=a.k, where=where, include=("distances",))  # noqa: E731
    filters = [
        ("eq", {"cat3": "b"}),
        ("in8", {"cat1000": {"$in": [f"v{i}" for i in range(0, 1000, 125)]}}),
        ("gt", {"x": {"$gt": 0.9}}),
        ("and_or_4_leaves", {"$and": [{"cat3": "a"}, {"$or": [{"x": {"$lt": 0.1}}, {"cat1000": "v7"}]}, {"x": {"$gte": 0.01}}]}),
    ]
    write_ids = [f"id{i}" for i in range(WRITE_ROWS)]
    write_mds = [metadata(i) for i in range(WRITE_ROWS)]
    write_vecs = np.random.default_rng(1000).standard_normal((CHUNK, a.dim)).astype(np.float32)[:WRITE_ROWS]   # (the rows they hold already)
    write = lambda col: col.upsert(ids=write_ids, embeddings=write_vecs, metadatas=write_mds)  # noqa: E731

    for name, where in filters:
        # the one-off build of the columns this filter names, measured on a collection that holds none
        device._drop_columns()
        keys = wc.filter_keys(where)
        build_ms, _ = timed(lambda: [device._engine.set_column(c.index, None, c.tags, c.cells) for c in (device._columns.build(k, device._metadatas) for k in keys)])
        got_host, got_device = ask(host, where), ask(device, where)
        assert got_host["ids"] == got_device["ids"] and np.array_equal(np.float32(got_host["distances"]).view(np.uint32),
                                                                        np.float32(got_device["distances"]).view(np.uint32)), name
        matched = int(host._where_mask(where).sum())
        first = {"host": [], "device": []}
        upsert = {"host": [], "device": []}
        encode = []
        for _ in range(a.writes):
            for route, col in (("host", host), ("device", device)):
                upsert[route].append(timed(lambda: write(col))[0])
                first[route].append(timed(lambda: ask(col, where))[0])
            encode.append(timed(lambda: device._columns.encode_slots(write_mds))[0])
        evals = device._engine.stat("where_evals")
        cached = {route: statistics.median(timed(lambda: ask(col, where))[0] for _ in range(a.reps)) for route, col in (("host", host), ("device", device))}
        assert device._engine.stat("where_evals") == evals, "the cached bitmap was not used"
        program = wc.compile_where(where, device._columns.by_key)
        call_ms = events(lambda: device._engine.eval_where(program))
        engine = device._engine
        prepared, bits = native.where_program(program), engine.eval_where(program)
        raw = lambda: native.check(engine._lib.codd_knn_eval_where(engine._h, ctypes.byref(prepared), bits.data_ptr(), bits.shape[0], engine._stream()), "eval_where")  # noqa: E731
        burst_ms = events(lambda: [raw() for _ in range(a.burst)]) / a.burst
        rows_now = engine.count()
        streamed = rows_now * 9 * len(program.columns())
        # an appending upsert: new ids, so the count and every column's mirrors grow
        append = {"host": [], "device": []}
        for w in range(a.writes):
            new_ids = [f"{name}-new{w}-{i}" for i in range(WRITE_ROWS)]
            for route, col in (("host", host), ("device", device)):
                append[route].append(timed(lambda: col.upsert(ids=new_ids, embeddings=write_vecs, metadatas=write_mds))[0])
        emit({**common, "point": "filter", "name": name, "where": where, "matched_rows": matched, "leaves": len(program.leaves),
              "distinct_columns": len(program.columns()), "first_after_write_host_ms_p50": statistics.median(first["host"]),
              "first_after_write_device_ms_p50": statistics.median(first["device"]), "cached_host_ms_p50": cached["host"],
              "cached_device_ms_p50": cached["device"], "eval_call_ms_p50": call_ms, "eval_back_to_back_ms": burst_ms, "burst": a.burst,
              "rows_at_eval": rows_now, "streamed_bytes": streamed,
              "back_to_back_fraction_of_hbm_peak": streamed / (burst_ms * 1e-3) / HBM_PEAK, "column_build_ms": build_ms,
              "columns_built": len(keys), "upsert_host_ms_p50": statistics.median(upsert["host"]),
              "upsert_device_ms_p50": statistics.median(upsert["device"]), "encode_ms_p50": statistics.median(encode),
              "append_host_ms_p50": statistics.median(append["host"]), "append_device_ms_p50": statistics.median(append["device"]),
              "columns_maintained": len(device._columns.device_columns())})


if __name__ == "__main__":
    main()
