#!/usr/bin/env python
"""Cost of the viewshed: which form of the sight lines is faster, how many steps the block maxima let it jump.

    python tools/viewshed_bench.py [--size 4096] [--observers 1,64] [--dists 256,1024,0] [--octaves 8] [--rounds 5]
        [--height-scale 64] [--eye 2]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's): the quantisation and the block maxima between device
events, then per number of observers (1: the centre; k^2: a k x k grid) and per distance limit (0: none) the sight lines in the
plain and the accel form, alternated in one process (plain, accel, plain, accel, ...) after one warm-up launch of each, which
also sizes the window: as many launches as fill about 0.3 s, 1 .. 10.  A time is the median of ``rounds`` windows between device
events, per launch.  The counts of the two forms are compared (``bit_identical``); the share of the cells that are seen and, from
ghm_viewshed_steps, the share of the plain form's steps that the accel form did not test are reported.  The faster form is what
viewshed.DEFAULT_ACCEL should say.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hydrology_bench import noise_terrain, stats      # noqa: E402


def stations(n, count):
    """``count`` observers on an n x n plane: the centre, or a k x k grid of cell centres"""
    k = int(round(count ** 0.5))
    if k * k != count:
        raise SystemExit("--observers takes squares (1, 4, 9, ..., 64, ...), got %d" % count)
    at = [int((i + 0.5) * n / k) for i in range(k)]
    return [(r, c) for r in at for c in at]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--observers", default="1,64")
    ap.add_argument("--dists", default="256,1024,0")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height-scale", type=float, default=64.0)
    ap.add_argument("--eye", type=float, default=2.0)
    a = ap.parse_args()
    from gan_heightmaps_amd import viewshed as VS
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    cells = n * n
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    elems = ops.viewshed_top_elems(n, n)
    d_h, d_z, d_c, d_t = dev.alloc(4 * cells), dev.alloc(4 * cells), dev.alloc(4 * cells), dev.alloc(4 * elems)
    dev.h2d(d_h, h)

    def window(fn, launches):
        dev.sync()
        dev.timer_start(0)
        for _ in range(launches):
            fn()
        dev.timer_stop(0)
        return dev.timer_ms(0) / launches                                # waits for the stop event

    quantise = lambda: ops.viewshed_quantise(d_h, n, n, n, a.height_scale, d_z, n)          # noqa: E731
    top = lambda: ops.viewshed_top(d_z, n, n, n, d_t, elems)                               # noqa: E731
    window(quantise, 1)
    window(top, 1)
    out = {"tool": "viewshed_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "block": VS.BLOCK,
           "height_scale": a.height_scale, "eye": a.eye, "default_accel": VS.DEFAULT_ACCEL,
           "quantise_ms": stats([window(quantise, 10) for _ in range(a.rounds)]),
           "top_ms": stats([window(top, 10) for _ in range(a.rounds)]), "sight": []}
    plane = np.empty((n, n), np.uint32)
    for count in [int(s) for s in a.observers.split(",")]:
        for dist in [float(s) for s in a.dists.split(",")]:
            sight = VS.Sight(eye_height=a.eye, max_dist=dist if dist > 0 else None, height_scale=a.height_scale)
            table = VS.observer_table(stations(n, count), sight, (n, n))

            def run(accel, steps=False):
                fn = ops.viewshed_steps if steps else ops.viewshed_sight
                fn(d_z, n, n, n, table, sight.target_q, accel, d_t if accel else None, d_c, n)

            def download():
                dev.sync()
                dev.d2h(plane, d_c, plane.nbytes)
                return plane.copy()
            launches, counts, tested = {}, {}, {}
            for accel in (False, True):                                  # warm-up: code objects loaded, clocks up; sizes the window
                ms = window(lambda: run(accel), 1)
                launches[accel] = int(min(10, max(1, 300.0 / max(ms, 1e-3))))
                counts[accel] = download()
            times = {False: [], True: []}
            for _ in range(a.rounds):
                for accel in (False, True):
                    times[accel].append(window(lambda: run(accel), launches[accel]))
            for accel in (False, True):
                run(accel, steps=True)
                tested[accel] = int(download().sum(dtype=np.uint64))
            r = {"observers": count, "max_dist": dist if dist > 0 else None, "plain_ms": stats(times[False]),
                 "accel_ms": stats(times[True]), "launches_per_window": [launches[False], launches[True]],
                 "bit_identical": bool(counts[False].tobytes() == counts[True].tobytes()),
                 "seen_share": round(float((counts[True] > 0).mean()), 5),
                 "plain_steps": tested[False], "accel_steps": tested[True],
                 "steps_skipped_share": round(1.0 - tested[True] / max(tested[False], 1), 5)}
            r["plain_over_accel"] = round(r["plain_ms"]["median"] / r["accel_ms"]["median"], 3)
            r["faster"] = "accel" if r["accel_ms"]["median"] < r["plain_ms"]["median"] else "plain"
            out["sight"].append(r)
            print("viewshed_bench: %d observers, max_dist %s: plain %.3f ms, accel %.3f ms" % (
                count, r["max_dist"], r["plain_ms"]["median"], r["accel_ms"]["median"]), file=sys.stderr, flush=True)
    dev.sync()
    for p in (d_h, d_z, d_c, d_t):
        dev.free(p)
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
