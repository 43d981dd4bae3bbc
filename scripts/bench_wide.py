#!/usr/bin/env python3
"""bench.py at the row widths of the wide-row kernels, one JSON line each (run on the GPU box).

    python scripts/bench_wide.py > profiles/wide/bench_wide.jsonl

1,536 and 3,072 f32 (the OpenAI embedders) at 10M rows; 4,096 f32 (LLM-based embedders) at 5M rows — 10M x 4,096 f32 plus its
shadows does not fit the 288 GB; 4,096 bf16 at 10M rows.  B = 256 takes the int8 filter: its roofline fraction is on the int8
shadow's bytes.  The script stops at the first run that fails or misses its correctness gate.  Extra bench.py arguments (e.g.
--set filter=0 --batch 8 for the wide exact scan) are passed on to every run.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [
    ("1536 f32, 10M rows", ["--dim", "1536", "--rows", "10000000"]),
    ("3072 f32, 10M rows", ["--dim", "3072", "--rows", "10000000"]),
    ("4096 f32, 5M rows", ["--dim", "4096", "--rows", "5000000"]),
    ("4096 bf16, 10M rows", ["--dim", "4096", "--rows", "10000000", "--dtype", "bf16"]),
]

for name, extra in RUNS:
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--warmup", "3", "--steps", "10", *extra, *sys.argv[1:]]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        # stop at the first failed run: a child that faulted or aborted may have left the card in a bad state, and no further
        # program is started on it
        print(json.dumps({"run": name, "failed": p.stderr[-500:], "returncode": p.returncode}), flush=True)
        sys.exit(1)
    line = json.loads(lines[-1])
    r = line["roofline"] or {}
    print(json.dumps({"run": name, "ms_per_step": line["ms_per_step"], "qps": line["value"], "results_valid": line["results_valid"],
                      "dominant_kernel": r.get("kernel"), "kernel_avg_ms": r.get("avg_launch_ms"), "achieved_GBps": r.get("achieved"),
                      "frac_of_8TBps": r.get("frac"), "bytes_are": r.get("algorithmic_bytes_are"), "all_kernels": r.get("all_kernels")}), flush=True)
    if not line["results_valid"]:
        sys.exit(1)
