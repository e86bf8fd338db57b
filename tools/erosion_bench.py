#!/usr/bin/env python
"""Cost of the erosion.  Two steps, each its own process so that each can run under its own time limit:

    python tools/erosion_bench.py kernels [--size 2304] [--iterations 32] [--rounds 5]
    python tools/erosion_bench.py world [--size 8192] [--iterations 32] [--dtype bf16x3]

kernels: the plain and the fused form of ghm_erosion_iterate on one size x size window of a seeded sine terrain, alternated
  in one process (plain, fused, plain, fused, ...), device events around each call of ``iterations`` steps after one warm-up
  call of each; per-iteration times, their ratio, and the bytes per cell per iteration each time amounts to.  The two final
  states are compared bit for bit.
world: a cold ``heightmap`` request of §4l's size x size rectangle of world 42 (default chunk_cells) on the eroded world
  against the same request on the raw world, in one process, each after a warm-up request that builds the plans; then the
  per-chunk split: device events around one trunk pass (_compute) and around one window's erosion (_erode).

Prints one JSON line per step."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(dev, fn):
    dev.timer_start(0)
    t0 = time.perf_counter()
    out = fn()
    dev.timer_stop(0)
    ms = dev.timer_ms(0)                                  # waits for the stop event
    return out, ms, (time.perf_counter() - t0) * 1e3


def sine_terrain(seed, n):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    z = np.zeros((n, n), np.float32)
    for o in range(5):
        th, ph = rng.uniform(0, 2 * np.pi, 2)
        z += np.float32(0.5 ** o) * np.sin(np.float32(2 * np.pi * 2 ** o / 384.0) * (np.float32(np.cos(th)) * y
                                                                                    + np.float32(np.sin(th)) * x) + ph)
    return np.clip(0.5 + 0.2 * z + 0.02 * rng.uniform(-1, 1, (n, n)), 0, 1).astype(np.float32)


def kernels(size, iterations, rounds):
    from gan_heightmaps_amd import erosion as ER
    from gan_heightmaps_amd.device import Device, Ops, erosion_params
    dev = Device(0)
    ops = Ops(dev)
    ero = ER.Erosion(iterations=iterations)
    params = erosion_params(**ero.as_dict())
    plane = 4 * size * size
    hm, s0, s1, tmp = dev.alloc(plane), dev.alloc(ER.PLANES * plane), dev.alloc(ER.PLANES * plane), dev.alloc(3 * plane)
    dev.h2d(hm, sine_terrain(1, size))
    times, finals = {False: [], True: []}, {}

    def once(fused):
        ops.erosion_init(hm, size, size, size, ero.height_scale, s0, size)
        dev.sync()
        fin, ms, _ = timed(dev, lambda: ops.erosion_iterate(params, s0, s1, tmp, size, size, size, iterations, fused))
        return fin, ms

    for fused in (False, True):                           # warm-up: code objects loaded, clocks up
        once(fused)
    for _ in range(rounds):
        for fused in (False, True):
            fin, ms = once(fused)
            times[fused].append(ms / iterations)
    for fused in (False, True):
        fin, _ = once(fused)
        finals[fused] = np.empty((ER.PLANES, size, size), np.float32)
        dev.d2h(finals[fused], fin, finals[fused].nbytes)
    cells = size * size

    def stats(v):
        v = sorted(v)
        med = v[len(v) // 2]
        return {"ms_per_iteration": {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)},
                "gb_per_s_at_14_planes": round(14 * 4 * cells / med / 1e6, 1),
                "bytes_per_cell_at_4_tb_per_s": round(med * 1e-3 * 4e12 / cells, 1)}
    res = {"tool": "erosion_bench", "step": "kernels", "size": size, "iterations": iterations, "rounds": rounds,
           "tile": list(ops.erosion_tile()), "plain": stats(times[False]), "fused": stats(times[True]),
           "bit_identical": bool(np.array_equal(finals[False], finals[True])),
           "ground_moved_max": float(np.abs(finals[True][0] / np.float32(ero.height_scale) - sine_terrain(1, size)).max())}
    res["plain_over_fused"] = round(res["plain"]["ms_per_iteration"]["median"] / res["fused"]["ms_per_iteration"]["median"], 3)
    dev.close()
    return res


def world(size, iterations, dtype):
    from gan_heightmaps_amd import erosion as ER
    from gan_heightmaps_amd.experiments import make_model
    from gan_heightmaps_amd.step import LANE_OF
    from gan_heightmaps_amd.world import erosion_sources
    model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=dtype)
    dev = model.engine.devs[LANE_OF['dcgan_gen']]
    ero = ER.Erosion(iterations=iterations)
    region = (-size // 2 + 37, -size // 2 - 101, size, size)          # §4l's rectangle: both signs, aligned to nothing
    hm = np.empty((1, size, size), np.float32)
    res = {"tool": "erosion_bench", "step": "world", "dtype": dtype, "size": size, "iterations": iterations, "halo": ero.halo}
    for name, kw in (("raw", {}), ("eroded", {"erosion": ero})):
        with model.terrain_world(42, **kw) as w:
            K = w.chunk_px
            w.heightmap(0, 0, K, K)                                   # warm-up: builds the plans, allocates the window
            w.clear()
            n, e = w.computed, w.eroded
            _, ms, wall = timed(dev, lambda: w.heightmap(*region, out=hm))
            res[name] = {"ms": round(ms, 2), "wall_ms": round(wall, 2), "mpix_per_s": round(size * size / ms / 1e3, 1),
                         "raw_chunks": w.computed - n, "erosions": w.eroded - e, "finite": bool(np.isfinite(hm).all())}
            if kw:
                # the per-chunk split, from a warm cache of raw chunks: one trunk pass, one window's erosion
                srcs = erosion_sources(0, 0, K, ero.halo)
                w._acquire([(0, 0)])
                trunk = sorted(timed(dev, lambda: w._cache.pool.append(w._compute(40, 40)))[1] for _ in range(5))
                erode = sorted(timed(dev, lambda: w._cache.pool.append(w._erode(srcs)))[1] for _ in range(5))
                res["per_chunk"] = {"chunk_px": K, "window_px": K + 2 * ero.halo,
                                    "trunk_ms": {"median": round(trunk[2], 3), "min": round(trunk[0], 3), "max": round(trunk[4], 3)},
                                    "erosion_ms": {"median": round(erode[2], 3), "min": round(erode[0], 3), "max": round(erode[4], 3)},
                                    "fused": bool(w._fused)}
                w._release()
    res["eroded_over_raw"] = round(res["eroded"]["ms"] / res["raw"]["ms"], 3)
    model.device.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["kernels", "world"])
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16x3")
    a = ap.parse_args()
    if a.step == "kernels":
        res = kernels(a.size or 2304, a.iterations, a.rounds)
    else:
        res = world(a.size or 8192, a.iterations, a.dtype)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
