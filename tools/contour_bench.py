#!/usr/bin/env python
"""Cost of the contours: what the count, the trace, the extraction and the marks take, and how much there is to trace.

    python tools/contour_bench.py [--size 4096] [--intervals 4,1] [--octaves 8] [--rounds 5] [--height-scale 64]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's), per interval (the other Levels at their defaults): the
quantisation once, then the count, the trace (links, both doublings, the lines' numbers and places), the extraction and the marks,
each between device events after one warm-up call; a time is the median of ``rounds`` calls.  The count and the trace wait for the
stream themselves (they return totals), so their times hold that wait; the extraction is followed by a sync inside its window.
The segments, lines, closed lines, vertices and the ranking's doubling rounds are reported with the bytes of the cells' buffer and
of the workspace.  There is one form, so nothing in the code depends on these numbers.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--intervals", default="4,1")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height-scale", type=float, default=64.0)
    a = ap.parse_args()
    from gan_heightmaps_amd import contour as CT
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    cells = n * n
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    d_h, d_z, d_m = dev.alloc(4 * cells), dev.alloc(4 * cells), dev.alloc(4 * cells)
    d_c = dev.alloc(ops.contour_cells_bytes(n, n))
    dev.h2d(d_h, h)

    def window(fn):
        dev.sync()
        dev.timer_start(0)
        fn()
        dev.timer_stop(0)
        return dev.timer_ms(0)                                           # waits for the stop event

    quantise = lambda: ops.viewshed_quantise(d_h, n, n, n, a.height_scale, d_z, n)          # noqa: E731
    window(quantise)
    out = {"tool": "contour_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "height_scale": a.height_scale,
           "cells_bytes": ops.contour_cells_bytes(n, n), "quantise_ms": stats([window(quantise) for _ in range(a.rounds)]),
           "levels": []}
    for interval in [float(s) for s in a.intervals.split(",")]:
        levels = CT.Levels(interval=interval, height_scale=a.height_scale)
        lv = (levels.base_q, levels.interval_q, -1)
        got = {}

        def count():
            got["S"] = ops.contour_count(d_z, n, n, n, *lv, d_c)

        window(count)
        S = got["S"]
        d_w = dev.alloc(ops.contour_workspace(n, n, S))

        def trace():
            got["L"], got["V"], got["rounds"] = ops.contour_trace(d_z, n, n, n, *lv, d_c, d_w, S)

        window(trace)
        L, V = got["L"], got["V"]
        arrays = [dev.alloc(max(b, 16)) for b in (12 * V, 8 * V, 8 * (L + 1), 4 * L, L)]

        def extract():
            ops.contour_extract(d_z, n, n, n, *lv, d_c, d_w, S, L, V, *arrays)
            dev.sync()

        marks = lambda: ops.contour_marks(d_z, n, n, n, *lv, levels.index_every, d_m, n)          # noqa: E731
        window(extract)
        window(marks)
        closed = np.empty(max(L, 1), np.uint8)
        if L:
            dev.d2h(closed, arrays[4], L)
        r = {"interval": interval, "segments": S, "lines": L, "closed": int(closed[:L].sum()), "vertices": V,
             "ranking_rounds": got["rounds"], "workspace_bytes": ops.contour_workspace(n, n, S)}
        for name, fn in (("count_ms", count), ("trace_ms", trace), ("extract_ms", extract), ("marks_ms", marks)):
            r[name] = stats([window(fn) for _ in range(a.rounds)])
        out["levels"].append(r)
        print("contour_bench: interval %g: %d segments, %d lines, %d vertices, %d rounds: count %.3f, trace %.3f, extract %.3f, "
              "marks %.3f ms" % (interval, S, L, V, got["rounds"], r["count_ms"]["median"], r["trace_ms"]["median"],
                                 r["extract_ms"]["median"], r["marks_ms"]["median"]), file=sys.stderr, flush=True)
        dev.sync()
        for p in arrays + [d_w]:
            dev.free(p)
    dev.sync()
    for p in (d_h, d_z, d_m, d_c):
        dev.free(p)
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
