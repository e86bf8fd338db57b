#!/usr/bin/env python
"""Cost of the sunlight: which form of the sun kernel is faster, how many steps the block maxima let it jump.

    python tools/sunlight_bench.py [--size 4096] [--octaves 8] [--rounds 5] [--height-scale 64] [--low 3] [--high 28]
        [--step-limit 120]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's) at the height scale: the quantisation, the block maxima
and their maximum once, then three suns -- ``Day()``, the default day of 24 positions; one position ``--high`` degrees up and one
``--low`` degrees up, both at azimuth 225 -- each in the plain and the accel form, alternated in one process (plain, accel, plain,
accel, ...) after one warm-up call of each, which also sizes the window: as many calls as fill about 0.3 s, 1 .. 10.  A time is
the median of ``rounds`` windows between device events, per call (a call is every launch of the sun's positions).  The planes of
the two forms are compared (``bit_identical``); the share of the (cell, position) pairs that are not lit (in shadow or
self-shaded) and, from ghm_sunlight_steps, the steps each form tested are reported.  The yardstick is the plain form in the same
process; the faster form under ``Day()`` is what sunlight.DEFAULT_FORM should say.  Every step runs under a limit of its own: a
step that takes longer than ``--step-limit`` seconds ends the process with a traceback.

Prints one JSON line."""
import argparse
import faulthandler
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hydrology_bench import noise_terrain, stats      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height-scale", type=float, default=64.0)
    ap.add_argument("--low", type=float, default=3.0)
    ap.add_argument("--high", type=float, default=28.0)
    ap.add_argument("--step-limit", type=float, default=120.0)
    a = ap.parse_args()
    from gan_heightmaps_amd import sunlight as SL
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    cells = n * n
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    elems = ops.viewshed_top_elems(n, n)
    sizes = [4 * cells] * 6 + [4 * elems, 4]
    d_h, d_z, d_l, d_m, d_q, d_e, d_t, d_x = bufs = [dev.alloc(b) for b in sizes]
    dev.h2d(d_h, h)

    def limited(fn, *args):
        faulthandler.dump_traceback_later(a.step_limit, exit=True)
        try:
            return fn(*args)
        finally:
            faulthandler.cancel_dump_traceback_later()

    def window(fn, launches):
        dev.sync()
        dev.timer_start(0)
        for _ in range(launches):
            fn()
        dev.timer_stop(0)
        return dev.timer_ms(0) / launches                                # waits for the stop event

    def prepare():
        ops.viewshed_quantise(d_h, n, n, n, a.height_scale, d_z, n)
        ops.viewshed_top(d_z, n, n, n, d_t, elems)
        ops.sunlight_zmax(d_t, elems, d_x)

    limited(window, prepare, 1)
    out = {"tool": "sunlight_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "height_scale": a.height_scale,
           "default_form": SL.DEFAULT_FORM, "prepare_ms": stats([limited(window, prepare, 5) for _ in range(a.rounds)]), "suns": []}
    plane = np.empty((n, n), np.uint32)
    suns = (("day", SL.Day().sun(height_scale=a.height_scale)), ("high", SL.Sun(((225.0, a.high),), height_scale=a.height_scale)),
            ("low", SL.Sun(((225.0, a.low),), height_scale=a.height_scale)))
    for label, sun in suns:
        table = sun.table()
        masked = len(table) <= 32

        def run(form, steps=False):
            top = d_t if form == 'accel' else None
            if steps:
                ops.sunlight_steps(d_z, n, n, n, table, sun.target_q, form == 'accel', top, d_x, d_l, n)
            else:
                ops.sunlight_sun(d_z, n, n, n, table, sun.target_q, form == 'accel', top, d_x, d_l, n, d_m if masked else None, n, d_q, n,
                                 d_e, n)

        def download(ptr):
            dev.sync()
            dev.d2h(plane, ptr, plane.nbytes)
            return plane.copy()
        launches, planes, tested = {}, {}, {}
        for form in SL.FORMS:                                            # warm-up: code objects loaded, clocks up; sizes the window
            ms = limited(window, lambda: run(form), 1)
            launches[form] = int(min(10, max(1, 300.0 / max(ms, 1e-3))))
            planes[form] = [download(p) for p in (d_l, d_q, d_e)]
        times = {form: [] for form in SL.FORMS}
        for _ in range(a.rounds):
            for form in SL.FORMS:
                times[form].append(limited(window, lambda: run(form), launches[form]))
        for form in SL.FORMS:
            limited(window, lambda: run(form, steps=True), 1)
            tested[form] = int(download(d_l).sum(dtype=np.uint64))
        r = {"sun": label, "positions": len(table), "reach": sun.reach, "plain_ms": stats(times['plain']), "accel_ms": stats(times['accel']),
             "launches_per_window": [launches[f] for f in SL.FORMS],
             "bit_identical": all(x.tobytes() == y.tobytes() for x, y in zip(planes['plain'], planes['accel'])),
             "not_lit_share": round(1.0 - float(planes['accel'][0].sum(dtype=np.uint64)) / (cells * len(table)), 5),
             "mean_hours": round(float(planes['accel'][1].mean()) / 256.0, 4),
             "plain_steps": tested['plain'], "accel_steps": tested['accel'],
             "steps_skipped_share": round(1.0 - tested['accel'] / max(tested['plain'], 1), 5)}
        r["plain_over_accel"] = round(r["plain_ms"]["median"] / r["accel_ms"]["median"], 3)
        r["faster"] = "accel" if r["accel_ms"]["median"] < r["plain_ms"]["median"] else "plain"
        out["suns"].append(r)
        print("sunlight_bench: %s, %d positions: plain %.3f ms, accel %.3f ms" % (
            label, len(table), r["plain_ms"]["median"], r["accel_ms"]["median"]), file=sys.stderr, flush=True)
    dev.sync()
    for p in bufs:
        dev.free(p)
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
