#!/usr/bin/env python
"""Throughput of TerrainWorld: the full-size test1_nobn_bilin_both generators (seeded weights), an 8192 x 8192
rectangle of world 42 at the default chunk size, against the finite-canvas path over the same area in the same process.

    python tools/world_bench.py [--size 8192] [--dtype bf16x3] [--profile DIR]

Prints one JSON line.  Every figure is device-event time around one whole call after a warm-up call (which builds the plans):
  (a) heightmap, cold cache, in Mpixel/s, beside generate_terrain on the same number of cells, with the expected cost ratio
      ((c s + 2 halo) / (c s))^2 trunk pixels per kept pixel against (band + 2 halo) / band;
  (b) both() at overlap 128, batch 4, cold cache, beside generate_terrain -> host -> texture_heightmap;
  (c) the same both() again from a warm cache, and shifted by half a chunk (the streaming case).
--profile DIR also runs (b) in a child process under ``rocprofv3 --kernel-trace --memory-copy-trace --stats`` and adds the
share of GPU time of the trunk, the U-Net, the four world kernels, the blend kernels and the copies."""
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


def timed(dev, fn):
    dev.timer_start(0)
    t0 = time.perf_counter()
    out = fn()
    wall = time.perf_counter() - t0
    dev.timer_stop(0)
    return out, dev.timer_ms(0), wall * 1e3


def run(size, dtype, only=None):
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd.step import LANE_OF
    from gan_heightmaps_amd.terrain import TerrainGeometry
    model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=dtype)
    dev = model.engine.devs[LANE_OF['dcgan_gen']]
    world = model.terrain_world(42, overlap=128, batch_size=4)
    geo, c, K = world.geometry, world.chunk_cells, world.chunk_px
    mpix = size * size / 1e6
    res = {"chunk_cells": c, "chunk_px": K, "halo": geo.halo, "size": size}
    region = (-size // 2 + 37, -size // 2 - 101, size, size)          # both signs, aligned to nothing
    hm = np.empty((geo.channels, size, size), np.float32)
    tex = np.empty((size, size, 3), np.uint8)

    cold = world.clear

    if only in (None, "b"):
        world.both(0, 0, 2 * K, 2 * K)                                # warm-up: builds the plans
    if only is None:
        cold()
        _, ms, wall = timed(dev, lambda: world.heightmap(*region, out=hm))
        res["a_heightmap_cold"] = {"ms": round(ms, 2), "wall_ms": round(wall, 2), "mpix_per_s": round(mpix / ms * 1e3, 2),
                                   "chunks": world.computed, "finite": bool(np.isfinite(hm).all())}
        cells = -(-size // geo.out)
        z = np.random.RandomState(0).rand(cells, cells, model.latent_dim).astype(np.float32)
        tg = TerrainGeometry(model.dcgan['gen'], cells, cells)
        ref = np.empty((geo.channels, tg.H, tg.W), np.float32)
        model.generate_terrain(z=z, out=ref)
        _, ms_t, wall_t = timed(dev, lambda: model.generate_terrain(z=z, out=ref))
        res["a_generate_terrain"] = {"cells": cells, "band": tg.band, "ms": round(ms_t, 2), "wall_ms": round(wall_t, 2),
                                     "mpix_per_s": round(tg.H * tg.W / ms_t / 1e3, 2)}
        res["a_cost_ratio"] = {"expected": round(((c * geo.s + 2 * geo.halo) / (c * geo.s)) ** 2
                                                 / ((tg.band + 2 * geo.halo) / tg.band), 3),
                               "measured": round((ms / mpix) / (ms_t / (tg.H * tg.W / 1e6)), 3)}
    if only in (None, "b"):
        cold()
        _, ms, wall = timed(dev, lambda: world.both(*region, out_heightmap=None, out_texture=tex, uint8=True))
        res["b_both_cold"] = {"ms": round(ms, 2), "wall_ms": round(wall, 2), "mpix_per_s": round(mpix / ms * 1e3, 2)}
    if only is None:
        def parent():
            model.generate_terrain(z=z, out=ref)
            return model.texture_heightmap(ref, overlap=128, batch_size=4, uint8=True)
        parent()
        _, ms_p, wall_p = timed(dev, parent)
        res["b_terrain_then_texture"] = {"ms": round(ms_p, 2), "wall_ms": round(wall_p, 2),
                                         "mpix_per_s": round(tg.H * tg.W / ms_p / 1e3, 2)}
        n = world.computed
        _, ms, wall = timed(dev, lambda: world.both(*region, out_texture=tex, uint8=True))
        res["c_both_warm"] = {"ms": round(ms, 2), "wall_ms": round(wall, 2), "mpix_per_s": round(mpix / ms * 1e3, 2),
                              "chunks_computed": world.computed - n}
        n = world.computed
        shifted = (region[0] + K // 2, region[1] + K // 2, size, size)
        _, ms, wall = timed(dev, lambda: world.both(*shifted, out_texture=tex, uint8=True))
        res["c_both_shifted_half_a_chunk"] = {"ms": round(ms, 2), "wall_ms": round(wall, 2),
                                              "mpix_per_s": round(mpix / ms * 1e3, 2), "chunks_computed": world.computed - n}
    world.close()
    model.device.close()
    return res


def profile_shares(outdir, size, dtype):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o",
           "world", "--", sys.executable, os.path.abspath(__file__), "--size", str(size), "--dtype", dtype, "--only", "b"]
    subprocess.check_call(cmd, timeout=1100)
    groups = {"conv": 0.0, "net_other": 0.0, "world_seed": 0.0, "world_emit": 0.0, "world_crop": 0.0, "world_gather": 0.0,
              "texture_blend": 0.0, "copies": 0.0}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name, ns = r["Name"], float(r["TotalDurationNs"])
            low = name.lower()
            key = next((k for k in ("world_seed", "world_emit", "world_crop", "world_gather") if k[6:] in name and "wld_" in name),
                       None)
            if key is None:
                key = "texture_blend" if ("tex_blend" in name or "tex_finalize" in name) else \
                    "conv" if ("conv" in low or "fanout" in low or "igemm" in low or "mfma" in low or "sp_" in name) \
                    else "net_other"
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
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--profile", default=None, help="directory for a rocprofv3 run of both() with a cold cache")
    ap.add_argument("--only", default=None, choices=["b"], help="run one case (the profiled child)")
    a = ap.parse_args()
    line = {"tool": "world_bench", "dtype": a.dtype, "results": run(a.size, a.dtype, a.only)}
    if a.profile:
        try:
            line["gpu_time_share"] = profile_shares(a.profile, a.size, a.dtype)
        except (OSError, subprocess.SubprocessError) as e:       # no profiler here: the timings still stand
            line["gpu_time_share"] = {"error": str(e)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
