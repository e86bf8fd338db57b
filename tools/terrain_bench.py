#!/usr/bin/env python
"""Throughput of Pix2Pix.generate_terrain: the full-size test1_nobn_bilin_both DCGAN generator (seeded
weights) on a 16 x 16 grid of latent vectors (an 8192 x 8192 heightmap), bilinear blend, the default band and band=4.

    python tools/terrain_bench.py [--cells 16] [--dtype bf16x3] [--profile DIR]

Prints one JSON line: per band, Mpixel/s of output from device events around the whole call (after one warm-up call), and
the host wall time.  --profile DIR also runs the default band in a child process under ``rocprofv3 --kernel-trace
--memory-copy-trace --stats`` and adds the share of GPU time taken by the convolutions, the other kernels of the head and
the trunk (BatchNorm, interleave, packing), the seed and emit kernels and the copies.  A z_fn_det run of 16 cells gives
the generator's per-sample throughput beside it."""
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


def run(cells, dtype, bands):
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd.step import LANE_OF
    from gan_heightmaps_amd.terrain import TerrainGeometry
    model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=dtype)
    dev = model.engine.devs[LANE_OF['dcgan_gen']]
    z = np.random.RandomState(0).rand(cells, cells, model.latent_dim).astype(np.float32)
    res = []
    for band in bands:
        geo = TerrainGeometry(model.dcgan['gen'], cells, cells, band)
        out = np.empty((geo.channels, geo.H, geo.W), np.float32)
        model.generate_terrain(z=z, band=band, out=out)                  # warm-up: builds the plans
        dev.timer_start(0)
        t0 = time.perf_counter()
        model.generate_terrain(z=z, band=band, out=out)
        wall = time.perf_counter() - t0
        dev.timer_stop(0)
        ms = dev.timer_ms(0)
        res.append({"band": geo.band, "halo": geo.halo, "windows": len(geo.windows), "ms": round(ms, 2),
                    "wall_ms": round(wall * 1e3, 2), "mpix_per_s": round(geo.H * geo.W / ms / 1e3, 2),
                    "finite": bool(np.isfinite(out).all()), "mean": round(float(out.mean()), 4),
                    "std": round(float(out.std()), 4)})
    # the same generator one 512 x 512 sample at a time (z_fn_det, batch 16): the per-cell cost without the canvas
    Z = z.reshape(-1, model.latent_dim)[:16]
    model.z_fn_det(Z)
    dev.timer_start(0)
    model.z_fn_det(Z)
    dev.timer_stop(0)
    ms = dev.timer_ms(0)
    res.append({"z_fn_det_batch": 16, "ms": round(ms, 2), "mpix_per_s": round(16 * 512 * 512 / ms / 1e3, 2)})
    model.device.close()
    return res


def profile_shares(outdir, cells, dtype):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o",
           "ter", "--", sys.executable, os.path.abspath(__file__), "--cells", str(cells), "--dtype", dtype, "--only", "0"]
    subprocess.check_call(cmd, timeout=1200)
    groups = {"trunk_conv": 0.0, "trunk_other": 0.0, "seed": 0.0, "emit": 0.0, "copies": 0.0}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name, ns = r["Name"], float(r["TotalDurationNs"])
            low = name.lower()
            key = "seed" if "ter_seed" in name else "emit" if "ter_emit" in name else \
                  "trunk_conv" if ("conv" in low or "fanout" in low or "igemm" in low or "mfma" in low or "sp_" in name) \
                  else "trunk_other"
            groups[key] += ns
    for f in glob.glob(os.path.join(outdir, "**", "*memory_copy_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            groups["copies"] += float(r["TotalDurationNs"])
    tot = sum(groups.values()) or 1.0
    out = {k: round(v / tot, 4) for k, v in groups.items()}
    out["total_ms"] = round(tot / 1e6, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=16)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--profile", default=None, help="directory for a rocprofv3 run of the default band")
    ap.add_argument("--only", type=int, default=None, help="run one band (0: the default; the profiled child)")
    a = ap.parse_args()
    bands = [None, 4]
    if a.only is not None:
        bands = [a.only or None]
    line = {"tool": "terrain_bench", "cells": a.cells, "dtype": a.dtype, "results": run(a.cells, a.dtype, bands)}
    if a.profile:
        try:
            line["gpu_time_share"] = profile_shares(a.profile, a.cells, a.dtype)
        except (OSError, subprocess.SubprocessError) as e:       # no profiler here: the timings still stand
            line["gpu_time_share"] = {"error": str(e)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
