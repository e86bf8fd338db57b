#!/usr/bin/env python
"""Cost of the sky-light bake: which of the two forms of ghm_skylight_bake is faster.

    python tools/skylight_bench.py [--size 4096] [--rounds 2] [--repeat 5] [--height-scale 64]
                                   [--directions 16 --steps 24 --step 1.5]

The plain and the tiled form on one size x size plane of a seeded sine terrain, alternated in one process (plain, tiled,
plain, tiled, ...) after one warm-up call of each; device events around ``repeat`` launches per window.  Per-launch times,
their ratio, the samples per second each amounts to, and whether the two planes are the same bits.  The faster form is what
skylight.DEFAULT_TILED should say.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sine_terrain(seed, n):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    z = np.zeros((n, n), np.float32)
    for o in range(5):
        th, ph = rng.uniform(0, 2 * np.pi, 2)
        z += np.float32(0.5 ** o) * np.sin(np.float32(2 * np.pi * 2 ** o / 384.0) * (np.float32(np.cos(th)) * y
                                                                                    + np.float32(np.sin(th)) * x) + ph)
    return np.clip(0.5 + 0.2 * z + 0.02 * rng.uniform(-1, 1, (n, n)), 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--height-scale", type=float, default=64.0)
    ap.add_argument("--directions", type=int, default=16)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--step", type=float, default=1.5)
    a = ap.parse_args()
    from gan_heightmaps_amd import skylight as SK
    from gan_heightmaps_amd.device import Device, Ops
    sky = SK.SkyLight(directions=a.directions, steps=a.steps, step=a.step)
    n = a.size
    dev = Device(0)
    ops = Ops(dev)
    if ops.skylight_lds_bytes(sky.reach) < 0:
        raise SystemExit("reach %d: the tiled form's window does not fit in LDS, there is nothing to compare" % sky.reach)
    src, out = dev.alloc(4 * n * n), dev.alloc(4 * n * n)
    dev.h2d(src, sine_terrain(1, n))

    def once(tiled, repeat):
        dev.sync()
        dev.timer_start(0)
        for _ in range(repeat):
            SK.bake_device(ops, src, n, n, sky, a.height_scale, out, tiled=tiled)
        dev.timer_stop(0)
        return dev.timer_ms(0) / repeat                    # waits for the stop event

    times, planes = {False: [], True: []}, {}
    for tiled in (False, True):                           # warm-up: code objects loaded, the table uploaded, clocks up
        once(tiled, 1)
    for _ in range(a.rounds):
        for tiled in (False, True):
            times[tiled].append(once(tiled, a.repeat))
    for tiled in (False, True):
        once(tiled, 1)
        planes[tiled] = np.empty((n, n), np.float32)
        dev.d2h(planes[tiled], out, planes[tiled].nbytes)
    samples = n * n * sky.directions * sky.steps

    def stats(v):
        v = sorted(v)
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        return {"ms": {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4), "runs": [round(x, 4) for x in v]},
                "gsamples_per_s": round(samples / med / 1e6, 1)}
    res = {"tool": "skylight_bench", "size": n, "rounds": a.rounds, "repeat": a.repeat, "height_scale": a.height_scale,
           "directions": sky.directions, "steps": sky.steps, "step": sky.step, "reach": sky.reach,
           "lds_bytes": ops.skylight_lds_bytes(sky.reach), "plain": stats(times[False]), "tiled": stats(times[True]),
           "bit_identical": bool(np.array_equal(planes[False], planes[True])),
           "mean": float(planes[False].mean()), "min": float(planes[False].min())}
    res["plain_over_tiled"] = round(res["plain"]["ms"]["median"] / res["tiled"]["ms"]["median"], 3)
    res["faster"] = "tiled" if res["plain_over_tiled"] > 1 else "plain"
    dev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
