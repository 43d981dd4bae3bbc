#!/usr/bin/env python3
"""Copies the summaries of scripts/profile_round.sh (gpurun_out/prof_<tag>, gpurun_out/pmc_<tag>) into profiles/<round>/ (development tool).

    python scripts/collect_profiles.py r3 [--prof gpurun_out/prof_r3 --pmc gpurun_out/pmc_r3]

Writes final_kernel_stats.csv, final_paired_bench_and_rocprof.json, bench_10m_with_cpu_comparators.json, i8_tile_pmc.txt (the tile kernels' counter means and the
figures derived from them), step_timeline_1p25m.txt, clustered_data_check.txt and profiles/traffic_<round>.json (FETCH_SIZE x 2 x 1024 bytes per row)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("round")
    p.add_argument("--prof")
    p.add_argument("--pmc")
    a = p.parse_args()
    prof = a.prof or os.path.join(ROOT, "gpurun_out", f"prof_{a.round}")
    pmc = a.pmc or os.path.join(ROOT, "gpurun_out", f"pmc_{a.round}")
    out = os.path.join(ROOT, "profiles", a.round)
    os.makedirs(out, exist_ok=True)
    # (gpurun merges every call's files into gpurun_out/: the newest trace is this run's)
    stats = max(glob.glob(os.path.join(prof, "trace", "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    shutil.copy(stats, os.path.join(out, "final_kernel_stats.csv"))
    rows = list(csv.DictReader(open(stats)))
    filt = [r for r in rows if re.search(r"i8_tile_kernel<0, ", r["Name"])]
    filt.sort(key=lambda r: -float(r["TotalDurationNs"]))
    f0 = filt[0]
    line = json.load(open(os.path.join(prof, "bench_paired.json")))
    kname = f0["Name"].split("(")[0].replace("void codd::", "")
    # the K timed launches inside the trace: the filter kernel's launches in start order are [priming search, W warm-up steps, K timed steps,
    # validation, latency and drop-in calls ...] (bench.py's order since round 3)
    trace = max(glob.glob(os.path.join(prof, "trace", "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    launches = sorted((r for r in csv.DictReader(open(trace)) if r["Kernel_Name"].startswith(f0["Name"].split("(")[0])), key=lambda r: int(r["Start_Timestamp"]))
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in launches]
    W, K = int(line["warmup"]), int(line["steps"])
    timed = durs[1 + W:1 + W + K]
    paired = {
        "_what": "python3 bench.py --full --no-cpu-baseline under `rocprofv3 --kernel-trace --stats` (scripts/profile_round.sh): the bench line and, in "
                 f"profiles/{a.round}/final_kernel_stats.csv, the per-kernel durations of the SAME run.  {kname}: {f0['Calls']} calls, average "
                 f"{float(f0['AverageNs']):,.0f} ns in the trace (warm-up, priming and validation launches included) vs roofline.avg_launch_ms below "
                 "(HIP events inside bench.py over the timed steps).  rocprof_timed_launches: the same K launches picked out of the kernel trace by position "
                 "(launch 1 = the priming search, then W warm-up steps, then the K timed steps) — the figure the event average has to agree with; the launches "
                 "behind them (validation, the drop-in call's batches of hashed text embeddings) run 5-12 % faster: quieter operand bytes, higher clock (DESIGN.md 11.6).",
        "rocprof_timed_launches": {"count": len(timed), "avg_ns": sum(timed) / max(len(timed), 1), "each_ns": timed},
        "rocprof_filter_kernel": {"name": kname, "calls": int(f0["Calls"]), "avg_ns": float(f0["AverageNs"]), "min_ns": float(f0["MinNs"]), "max_ns": float(f0["MaxNs"])},
        "bench_line": line,
    }
    json.dump(paired, open(os.path.join(out, "final_paired_bench_and_rocprof.json"), "w"), indent=1)
    shutil.copy(os.path.join(prof, "bench_full.json"), os.path.join(out, "bench_10m_with_cpu_comparators.json"))
    for src, dst in (("step_timeline_1p25m.txt", "step_timeline_1p25m.txt"), ("clustered.txt", "clustered_data_check.txt")):
        if os.path.exists(os.path.join(prof, src)):
            shutil.copy(os.path.join(prof, src), os.path.join(out, dst))
    # counters: the tile kernels only
    summ = open(os.path.join(pmc, "summary.txt")).read().splitlines()
    keep = [l for l in summ if "i8_tile_kernel" in l or "finalize_fb_kernel" in l or "anchor_thr_kernel" in l]
    vals = {}
    for l in keep:
        m = re.match(r"(i8_tile_kernel<0, [^>]*>)\s+(\S+)\s+n=\s*(\d+)\s+mean=(\S+)", l)
        if m and int(m.group(3)) >= 5:
            vals.setdefault(m.group(1), {})[m.group(2)] = float(m.group(4))
    notes = []
    traffic = None
    for k, v in vals.items():
        if "GRBM_GUI_ACTIVE" in v and "SQ_VALU_MFMA_BUSY_CYCLES" in v:
            cyc = v["GRBM_GUI_ACTIVE"] / 8
            notes.append(f"#   {k}: GRBM_GUI_ACTIVE / 8 XCDs = {cyc:.3e} cycles per launch; matrix pipe busy {v['SQ_VALU_MFMA_BUSY_CYCLES']:.3e} / (1024 SIMDs x cycles) = "
                         f"{100 * v['SQ_VALU_MFMA_BUSY_CYCLES'] / (1024 * cyc):.1f} %; waves parked (SQ_WAIT_ANY / SQ_WAVE_CYCLES) {100 * v.get('SQ_WAIT_ANY', 0) / max(v.get('SQ_WAVE_CYCLES', 1), 1):.1f} %; "
                         f"non-MFMA vector instructions {(v.get('SQ_INSTS_VALU', 0) - v.get('SQ_INSTS_MFMA', 0)):.3e} = {(v.get('SQ_INSTS_VALU', 0) - v.get('SQ_INSTS_MFMA', 0)) / max(v.get('SQ_INSTS_MFMA', 1), 1):.2f} per MFMA; "
                         f"LDS bank conflict cycles {v.get('SQ_LDS_BANK_CONFLICT', 0):.3e}")
        if "FETCH_SIZE" in v:
            gb = v["FETCH_SIZE"] * 1024 * 2 / 1e9
            notes.append(f"#   {k}: FETCH_SIZE {v['FETCH_SIZE']:.4e} KiB x 1024 x 2 (gfx950: a 16-B/lane coalesced stream reads as half) = {gb:.3f} GB per launch")
            if traffic is None or v["FETCH_SIZE"] > traffic[1]:
                traffic = (k, v["FETCH_SIZE"])
    with open(os.path.join(out, "i8_tile_pmc.txt"), "w") as f:
        f.write("# rocprofv3 --pmc <counters> --kernel-trace -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --latency-iters 3   (scripts/pmc_round.sh; three separate\n"
                "# passes: SQ set 1 | SQ set 2 | GRBM_GUI_ACTIVE + FETCH_SIZE).  10M x 768 fp32 corpus, B = 256 steps (+ B = 1 latency calls); means per launch.\n")
        f.write("\n".join(keep) + "\n# derived:\n" + "\n".join(notes) + "\n")
    if traffic:
        rows_n = line["config"]["rows"]
        prev = {}
        for name in ("traffic_r2.json", "traffic_r1.json"):
            try:
                prev = json.load(open(os.path.join(ROOT, "profiles", name)))
                break
            except OSError:
                continue
        bpr = dict(prev.get("bytes_per_row", {}))
        bpr["filter8"] = {"f32": traffic[1] * 2048 / rows_n}
        json.dump({"_source": f"profiles/{a.round}/i8_tile_pmc.txt ({traffic[0]}, rocprofv3 --pmc FETCH_SIZE, separate pass, 10M x 768, B = 256); the other kernels as in the earlier rounds' files",
                   "_correction": "FETCH_SIZE is KiB and reads 1/2 of a 16-B/lane coalesced stream on gfx950: bytes = 2*1024*FETCH_SIZE",
                   "dim": line["config"]["dim"], "bytes_per_row": bpr,
                   "source": f"rocprofv3 --pmc FETCH_SIZE pass of round {a.round[1:]}, x2 x1024: profiles/{a.round}/i8_tile_pmc.txt"},
                  open(os.path.join(ROOT, "profiles", f"traffic_{a.round}.json"), "w"), indent=1)
    print("\n".join(notes))
    print("filter kernel in the trace:", kname, f0["Calls"], f0["AverageNs"], "events:", line["roofline"]["avg_launch_ms"])


if __name__ == "__main__":
    main()
