#!/usr/bin/env python
"""Throughput of Pix2Pix.texture_heightmap: the full-size test1_nobn_bilin_both U-Net (seeded weights) on an
8192 x 8192 uint8 heightmap, overlap 0 and 128, batch_size 4 and 8.

    python tools/texture_bench.py [--size 8192] [--dtype bf16x3] [--profile DIR]

Prints one JSON line: per configuration, Mpixel/s of canvas from device events around the whole call (after one warm-up
call), and the host wall time.  --profile DIR also runs one configuration (overlap 128, batch 4) in a child process under
``rocprofv3 --kernel-trace --memory-copy-trace --stats`` and adds the share of GPU time taken by the U-Net forward,
gather, blend, finalize and the copies."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def heightmap(n, seed=0):
    """a smooth random uint8 heightmap (sum of a few sinusoids), like a DEM rather than noise"""
    rng = np.random.RandomState(seed)
    y = np.linspace(0, 1, n, dtype=np.float32)[:, None]
    x = np.linspace(0, 1, n, dtype=np.float32)[None, :]
    h = np.zeros((n, n), np.float32)
    for k in range(6):
        fy, fx, ph = rng.uniform(1, 12, 3)
        h += np.sin(2 * np.pi * (fy * y + fx * x) + ph) / (k + 1)
    h = (h - h.min()) / (h.max() - h.min())
    return (h * 255).astype(np.uint8)


def run(size, dtype, configs):
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd.step import LANE_OF
    model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=dtype)
    dev = model.engine.devs[LANE_OF['p2p_gen']]
    x = heightmap(size)
    out = np.empty((size, size, 3), np.uint8)
    res = []
    for o, b in configs:
        model.texture_heightmap(x, overlap=o, batch_size=b, out=out, uint8=True)      # warm-up: builds the plan
        dev.timer_start(0)
        t0 = time.perf_counter()
        model.texture_heightmap(x, overlap=o, batch_size=b, out=out, uint8=True)
        wall = time.perf_counter() - t0
        dev.timer_stop(0)
        ms = dev.timer_ms(0)
        res.append({"overlap": o, "batch_size": b, "ms": round(ms, 2), "wall_ms": round(wall * 1e3, 2),
                    "mpix_per_s": round(size * size / ms / 1e3, 2)})
    model.device.close()
    return res


def profile_shares(outdir, size, dtype):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "tex", "--",
           sys.executable, os.path.abspath(__file__), "--size", str(size), "--dtype", dtype, "--only", "128,4"]
    subprocess.check_call(cmd, timeout=1200)
    groups = {"unet_forward": 0.0, "gather": 0.0, "blend": 0.0, "finalize": 0.0, "copies": 0.0}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name, ns = r["Name"], float(r["TotalDurationNs"])
            key = "gather" if "tex_gather" in name else "blend" if "tex_blend" in name else \
                  "finalize" if "tex_finalize" in name else "unet_forward"
            groups[key] += ns
    for f in glob.glob(os.path.join(outdir, "**", "*memory_copy_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            groups["copies"] += float(r["TotalDurationNs"])
    tot = sum(groups.values()) or 1.0
    return {k: round(v / tot, 4) for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--profile", default=None, help="directory for a rocprofv3 run of (overlap 128, batch 4)")
    ap.add_argument("--only", default=None, help="o,b: run one configuration (the profiled child)")
    a = ap.parse_args()
    configs = [(0, 4), (0, 8), (128, 4), (128, 8)]
    if a.only:
        o, b = (int(v) for v in a.only.split(","))
        configs = [(o, b)]
    line = {"tool": "texture_bench", "size": a.size, "dtype": a.dtype, "results": run(a.size, a.dtype, configs)}
    if a.profile:
        try:
            line["gpu_time_share"] = profile_shares(a.profile, a.size, a.dtype)
        except (OSError, subprocess.SubprocessError) as e:       # no profiler here: the timings still stand
            line["gpu_time_share"] = {"error": str(e)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
