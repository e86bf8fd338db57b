#!/usr/bin/env python
"""Cost of the climate: what the transport takes in both forms under every wind, and the spread, the temperature and
biome launch and the discharge beside it.

    python tools/climate_bench.py [--size 4096] [--winds N,NE,E,SE,S,SW,W,NW] [--octaves 8] [--rounds 5] [--check]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's) under the default weather: per wind the transport in the
``line`` and the ``staged`` form, each between device events on the launch's stream; the two forms are alternated call by
call in this one process, after a warm-up call of each, so that neither has the warmer device; a time is the median of ``rounds``
calls.  Then, once, the spread, the temperature and biome launch, and the discharge over the directions of the plane's own hydrology
(it waits for the stream itself).  --check compares the two forms' planes on the host, wind by wind.  climate.DEFAULT_FORM is the form
whose transport was the faster here summed over the winds.

Prints one JSON line per wind and one for the other steps."""
import argparse
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
    ap.add_argument("--winds", default="N,NE,E,SE,S,SW,W,NW")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    from gan_heightmaps_amd import climate as CL
    from gan_heightmaps_amd import hydrology as HY
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    dev = Device(0)
    ops = Ops(dev)
    h = np.clip(np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32), 0, 1)
    weather, biomes = CL.Weather(), CL.Biomes()
    q = weather.quantised()
    zq = np.rint(h * np.float32(weather.height_scale * 256.0)).astype(np.int32)
    d_z, d_raw, d_rain, d_t, d_b = (dev.alloc(4 * n * n) for _ in range(5))
    dev.h2d(d_z, zq)

    def window(fn):
        dev.sync()
        dev.timer_start(0)
        fn()
        dev.timer_stop(0)
        return dev.timer_ms(0)                                           # waits for the stop event

    def transport(wind, form):
        ops.climate_transport(d_z, n, n, n, CL.WINDS.index(wind), CL.FORMS.index(form), q['sea_q'], q['hum_q'], q['evap_q'], q['base_q'],
                              q['up_q'], q['rec_q'], d_raw, n)

    total = {form: 0.0 for form in CL.FORMS}
    for wind in a.winds.split(","):
        times = {form: [] for form in CL.FORMS}
        for i in range(a.rounds + 1):                                    # the first call of each form is the warm-up
            for form in CL.FORMS:
                times[form].append(window(lambda: transport(wind, form)))
        r = {"tool": "climate_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "wind": wind, "default_form": CL.DEFAULT_FORM}
        for form in CL.FORMS:
            r["transport_%s_ms" % form] = stats(times[form][1:])
            total[form] += r["transport_%s_ms" % form]["median"]
        if a.check:
            planes = []
            for form in CL.FORMS:
                transport(wind, form)
                dev.sync()
                planes.append(np.empty((n, n), np.uint32))
                dev.d2h(planes[-1], d_raw, planes[-1].nbytes)
            r["forms_equal"] = bool(np.array_equal(*planes))
        print("climate_bench: wind %s: transport %.3f line and %.3f staged ms" % (wind, r["transport_line_ms"]["median"],
                                                                                 r["transport_staged_ms"]["median"]), file=sys.stderr, flush=True)
        print(json.dumps(r), flush=True)

    def spread():
        ops.climate_spread(d_raw, n, n, n, q['spread'], d_rain, n)

    def chart():
        ops.climate_biome(d_z, n, d_rain, n, n, n, q['sea_q'], q['t0_q'], q['lapse_q'], q['lat_q'], 0, *biomes.quantised(), biomes.ocean, d_t, n,
                          d_b, n)

    r = {"tool": "climate_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "spread": q['spread'],
         "transport_sum_ms": total, "workspace_bytes": ops.climate_workspace(n, n)}
    for name, fn in (("spread", spread), ("biome", chart)):
        window(fn)
        r[name + "_ms"] = stats([window(fn) for _ in range(a.rounds)])
    hydro = HY.analyse(ops, h, keep=('direction',))
    d_dir, d_q, d_e, d_w = dev.alloc(n * n), dev.alloc(8 * n * n), dev.alloc(4 * n * n), dev.alloc(ops.climate_workspace(n, n))
    dev.h2d(d_dir, hydro.direction)
    got = {}

    def discharge():
        got["rounds"] = ops.climate_discharge(d_dir, n, d_rain, n, n, n, q['ref_q'], d_q, n, d_e, n, d_w)

    window(discharge)
    r["discharge_ms"] = stats([window(discharge) for _ in range(a.rounds)])
    r["discharge_rounds"] = got["rounds"]
    print("climate_bench: transport over the winds %.3f line and %.3f staged, spread %.3f, temperature and biome %.3f, discharge %.3f ms "
          "(%d rounds)" % (total['line'], total['staged'], r["spread_ms"]["median"], r["biome_ms"]["median"], r["discharge_ms"]["median"],
                           got["rounds"]), file=sys.stderr, flush=True)
    print(json.dumps(r), flush=True)
    dev.sync()
    for p in (d_z, d_raw, d_rain, d_t, d_b, d_dir, d_q, d_e, d_w):
        dev.free(p)
    dev.close()


if __name__ == "__main__":
    main()
