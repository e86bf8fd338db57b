#!/usr/bin/env python
"""Cost of the scatter: which form of the thinning is faster, how many sweeps it takes, and what the other stages cost.

    python tools/scatter_bench.py [--size 4096] [--spacings 2,8,32] [--densities 1.0,0.1] [--octaves 8] [--rounds 3]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's), with a habitat that takes every altitude and slope
so that the density alone thins the candidates: the chance and the candidates launches between device events (the median of
``rounds`` windows of ten launches), then per spacing and density the thinning in the plain and the tiled form, alternated in one
process (plain, tiled, plain, tiled, ...) after one warm-up run of each.  A thinning waits for the device once per group of
sweeps, so its time is the host clock's around the call, from an idle device to an idle device; the candidates launch puts the
state plane back before each run and is not counted.  The planes of the two forms are compared, and checked for the two
invariants on a corner of the plane.  Then the download of the state plane and the collection of the points on the host.  What
the tiled form's empty-tile skip is worth shows against a tuning build with GHM_BUILD_DEFINES=-DGHM_SCATTER_NO_SKIP.  The faster
form is what scatter.DEFAULT_TILED should say.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hydrology_bench import noise_terrain, stats      # noqa: E402


def conflicts(state, s2):
    """pairs of kept cells with dy^2 + dx^2 < s2 in a plane (small: the host does this)"""
    kept = state == 2
    R = 0
    while (R + 1) * (R + 1) < s2:
        R += 1
    H, W = kept.shape
    n = 0
    for dy in range(0, R + 1):
        for dx in range(-R, R + 1):
            if (dy == 0 and dx <= 0) or dy * dy + dx * dx >= s2:
                continue
            a = kept[:H - dy, max(0, -dx):W - max(0, dx)]
            b = kept[dy:, max(0, dx):W - max(0, -dx)]
            n += int((a & b).sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--spacings", default="2,8,32")
    ap.add_argument("--densities", default="1.0,0.1")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from gan_heightmaps_amd import scatter as SC
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    cells = n * n
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    d_h, d_c, d_p = (dev.alloc(4 * cells) for _ in range(3))
    d_s, d_t, ws = dev.alloc(cells), dev.alloc(4 * 384), dev.alloc(ops.scatter_workspace(n, n))
    dev.h2d(d_h, h)

    def window(fn, launches=10):
        dev.sync()
        dev.timer_start(0)
        for _ in range(launches):
            fn()
        dev.timer_stop(0)
        return dev.timer_ms(0) / launches                                # waits for the stop event

    out = {"tool": "scatter_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "tile": 32,
           "default_tiled": SC.DEFAULT_TILED, "no_skip_build": "GHM_SCATTER_NO_SKIP" in os.environ.get("GHM_BUILD_DEFINES", ""),
           "thin": []}
    state = np.empty((n, n), np.uint8)
    for density in [float(s) for s in a.densities.split(",")]:
        hab = SC.Habitat(altitude=(-10.0, 10.0), slope=(0.0, 90.0), density=density)
        dev.h2d(d_t, hab.tables())
        chance = lambda: ops.scatter_chance(d_h, n, n, n, d_t, 64.0, density, d_c, n)                  # noqa: E731
        cand = lambda: ops.scatter_candidates(d_c, n, n, n, 1, (0, 0), d_s, n, d_p, n)                 # noqa: E731
        window(chance)
        window(cand)
        stage = {"density": density, "chance_ms": stats([window(chance) for _ in range(a.rounds)]),
                 "candidates_ms": stats([window(cand) for _ in range(a.rounds)])}
        out.setdefault("stages", []).append(stage)
        for spacing in [float(s) for s in a.spacings.split(",")]:
            s2 = SC.Species("bench", spacing).s2

            def thin(tiled):
                cand()
                dev.sync()
                t0 = time.perf_counter()
                sweeps = ops.scatter_thin(d_p, n, d_s, n, n, n, s2, tiled, ws)
                dev.sync()
                return (time.perf_counter() - t0) * 1e3, sweeps
            times, sweeps, planes = {False: [], True: []}, {}, {}
            for tiled in (False, True):                                  # warm-up: code objects loaded, clocks up
                _, sweeps[tiled] = thin(tiled)
                dev.d2h(state, d_s, cells)
                planes[tiled] = state.copy()
            for _ in range(a.rounds):
                for tiled in (False, True):
                    times[tiled].append(thin(tiled)[0])
            t0 = time.perf_counter()
            dev.d2h(state, d_s, cells)
            t1 = time.perf_counter()
            points = np.argwhere(state == 2)
            t2 = time.perf_counter()
            corner = planes[True][:512, :512]
            r = {"density": density, "spacing": spacing, "s2": s2, "plain_ms": stats(times[False]), "tiled_ms": stats(times[True]),
                 "plain_sweeps": sweeps[False], "tiled_launches": sweeps[True], "lds_bytes": ops.scatter_lds_bytes(s2),
                 "candidates": int((planes[True] != 0).sum()), "points": int(len(points)),
                 "download_ms": round((t1 - t0) * 1e3, 3), "collect_ms": round((t2 - t1) * 1e3, 3),
                 "bit_identical": bool(planes[False].tobytes() == planes[True].tobytes()),
                 "undecided": int((planes[True] == 1).sum()), "corner_conflicts": conflicts(corner, s2)}
            r["plain_over_tiled"] = round(r["plain_ms"]["median"] / r["tiled_ms"]["median"], 3)
            r["faster"] = "tiled" if r["tiled_ms"]["median"] < r["plain_ms"]["median"] else "plain"
            out["thin"].append(r)
    dev.sync()
    for p in (d_h, d_c, d_p, d_s, d_t, ws):
        dev.free(p)
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
