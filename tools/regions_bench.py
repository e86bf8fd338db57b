#!/usr/bin/env python
"""Cost of the regions: what the labelling in both forms, the count, the trace, the extraction and the host's assembly
take, and how many edges, rings, polygons and rounds there are.

    python tools/regions_bench.py [--size 4096] [--planes land,bands] [--octaves 8] [--rounds 5] [--sea-level 0.5]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's), as ``land`` above the sea level and as ``bands`` of the
default contour levels: the labelling, the count, the trace and the extraction, each between device events after one warm-up call;
a time is the median of ``rounds`` calls.  The labelling, the count and the trace wait for the stream themselves (they return
totals), so their times hold that wait; the extraction is followed by a sync inside its window.  The two forms of the labelling
are alternated call by call in this one process, after a warm-up call of each, so that neither has the warmer device.  The host's
assembly (``regions.report``: the points, the perimeters, the boxes) is timed on the host clock.  regions.DEFAULT_FORM is the form
whose labelling was the faster here on the ``bands`` plane.

Prints one JSON line per plane."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--planes", default="land,bands")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sea-level", type=float, default=0.5)
    a = ap.parse_args()
    from gan_heightmaps_amd import regions as RG
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    dev = Device(0)
    ops = Ops(dev)
    h = np.clip(np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32), 0, 1)
    d_l, d_c, d_p = dev.alloc(4 * n * n), dev.alloc(4 * n * n), dev.alloc(4 * n * n)
    d_w = dev.alloc(ops.regions_workspace(n, n))

    def window(fn):
        dev.sync()
        dev.timer_start(0)
        fn()
        dev.timer_stop(0)
        return dev.timer_ms(0)                                           # waits for the stop event

    for plane in a.planes.split(","):
        labels = RG.land(h, a.sea_level) if plane == "land" else RG.bands(h)
        dev.h2d(d_l, labels)
        got = {}

        def label(form):
            got["sweeps_" + form] = ops.regions_label(d_l, n, n, n, RG.FORMS.index(form), d_c, n, d_w)

        times = {form: [] for form in RG.FORMS}
        for i in range(a.rounds + 1):                                    # the first call of each form is the warm-up
            for form in RG.FORMS:
                times[form].append(window(lambda: label(form)))
        r = {"tool": "regions_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "plane": plane,
             "labels": int(labels.max()) + 1, "workspace_bytes": ops.regions_workspace(n, n), "default_form": RG.DEFAULT_FORM}
        for form in RG.FORMS:
            r["label_%s_ms" % form] = stats(times[form][1:])
            r["sweeps_" + form] = got["sweeps_" + form]

        def count():
            got["counts"] = ops.regions_count(d_l, n, d_c, n, n, n, d_w)

        window(count)
        r["count_ms"] = stats([window(count) for _ in range(a.rounds)])
        E, P = got["counts"]
        r["edges"], r["polygons"], r["trace_bytes"] = E, P, ops.regions_trace_bytes(E)
        d_t = dev.alloc(max(r["trace_bytes"], 16))

        def trace():
            got["trace"] = ops.regions_trace(n, n, d_w, d_t, E, P)

        window(trace)
        r["trace_ms"] = stats([window(trace) for _ in range(a.rounds)])
        R, V, rounds = got["trace"]
        r["rings"], r["vertices"], r["trace_rounds"] = R, V, rounds
        host = (np.empty(V, np.int32), np.empty(R + 1, np.int64), np.empty(R, np.int32), np.empty(R, np.uint8), np.empty(P, np.int32),
                np.empty(P, np.int32), np.empty(P, np.uint32))
        arrays = [dev.alloc(max(x.nbytes, 16)) for x in host]

        def extract():
            ops.regions_extract(d_l, n, d_c, n, n, n, d_w, d_t, E, P, R, V, *arrays, d_p, n)
            dev.sync()

        window(extract)
        r["extract_ms"] = stats([window(extract) for _ in range(a.rounds)])
        for x, p in zip(host, arrays):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        t0 = time.perf_counter()
        found = RG.report(*host, RG.Areas(), (0, 0), (n, n))
        r["assembly_host_ms"] = (time.perf_counter() - t0) * 1e3
        r["holes"] = int(found.hole.sum())
        print("regions_bench: %s: %d edges, %d rings, %d polygons, %d vertices, %d rounds: label %.3f sweep (%d sweeps) and %.3f union, "
              "count %.3f, trace %.3f, extract %.3f, assembly (host) %.1f ms" % (
                  plane, E, R, P, V, rounds, r["label_sweep_ms"]["median"], r["sweeps_sweep"], r["label_union_ms"]["median"],
                  r["count_ms"]["median"], r["trace_ms"]["median"], r["extract_ms"]["median"], r["assembly_host_ms"]), file=sys.stderr, flush=True)
        print(json.dumps(r), flush=True)
        dev.sync()
        for p in [d_t] + arrays:
            dev.free(p)
    dev.sync()
    for p in (d_l, d_c, d_p, d_w):
        dev.free(p)
    dev.close()


if __name__ == "__main__":
    main()
