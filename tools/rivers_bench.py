#!/usr/bin/env python
"""Cost of the rivers: what the count, the trace in both forms, the extraction and the host's orders take, and how many
cells, reaches and vertices there are to trace.

    python tools/rivers_bench.py [--size 4096] [--thresholds 256,16] [--octaves 8] [--rounds 5]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's) through ``hydrology.analyse``: per threshold the count,
the trace, and the extraction, each between device events after one warm-up call; a time is the median of ``rounds`` calls.  The
count and the trace wait for the stream themselves (they return totals), so their times hold that wait; the extraction is followed
by a sync inside its window.  The two forms of the trace are alternated call by call in this one process, after a warm-up call of
each, so that neither has the warmer device.  The orders are timed on the host clock.  rivers.DEFAULT_FORM is the form whose trace
was the faster here at a threshold of 256.

Prints one JSON line per threshold."""
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
    ap.add_argument("--thresholds", default="256,16")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from gan_heightmaps_amd import hydrology as HY
    from gan_heightmaps_amd import rivers as RV
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    hydro = HY.analyse(ops, h, keep=('direction', 'accumulation'))
    d_dir, d_kind, d_acc = dev.alloc(n * n), dev.alloc(n * n), dev.alloc(4 * n * n)
    d_w = dev.alloc(ops.rivers_workspace(n, n))
    dev.h2d(d_dir, hydro.direction)
    dev.h2d(d_acc, hydro.accumulation)

    def window(fn):
        dev.sync()
        dev.timer_start(0)
        fn()
        dev.timer_stop(0)
        return dev.timer_ms(0)                                           # waits for the stop event

    for T in (int(t) for t in a.thresholds.split(",")):
        got = {}

        def count():
            got["counts"] = ops.rivers_count(d_dir, n, d_acc, n, n, n, T, d_kind, n, d_w)

        window(count)
        r = {"tool": "rivers_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "threshold": T,
             "workspace_bytes": ops.rivers_workspace(n, n), "count_ms": stats([window(count) for _ in range(a.rounds)])}
        cells, R = got["counts"][:2]
        r.update(zip(("cells", "reaches", "sources", "confluences", "mouths", "isolated"), got["counts"]))
        r["list_bytes"] = ops.rivers_list_bytes(cells)
        d_l = dev.alloc(max(r["list_bytes"], 16))

        def trace(form):
            got["V"], got["trace_rounds"] = ops.rivers_trace(d_dir, n, d_kind, n, n, n, RV.FORMS.index(form), d_w,
                                                             d_l if form == "list" else None, cells, R)

        times = {form: [] for form in RV.FORMS}
        for i in range(a.rounds + 1):                                    # the first call of each form is the warm-up
            for form in RV.FORMS:
                times[form].append(window(lambda: trace(form)))
        for form in RV.FORMS:
            r["trace_%s_ms" % form] = stats(times[form][1:])
        V = got["V"]
        r["vertices"], r["trace_rounds"] = V, got["trace_rounds"]
        host = (np.empty(V, np.int32), np.empty(R + 1, np.int64), np.empty(R, np.int32))
        arrays = [dev.alloc(max(x.nbytes, 16)) for x in host]

        def extract():                                                   # the last trace was the list form's
            ops.rivers_extract(d_dir, n, d_kind, n, n, n, d_w, d_l, cells, R, V, *arrays)
            dev.sync()

        window(extract)
        r["extract_ms"] = stats([window(extract) for _ in range(a.rounds)])
        for x, p in zip(host, arrays):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        area = RV.reach_areas(host[0], host[1], host[2], hydro.direction, hydro.accumulation)
        t0 = time.perf_counter()
        order, _, _ = ops.rivers_order(host[2], area)
        r["order_host_ms"] = (time.perf_counter() - t0) * 1e3
        r["greatest_order"] = int(order.max()) if R else 0
        print("rivers_bench: T = %d: %d cells, %d reaches, %d vertices, %d rounds, order up to %d: count %.3f, trace %.3f plain and "
              "%.3f list, extract %.3f, orders (host) %.3f ms" % (
                  T, cells, R, V, r["trace_rounds"], r["greatest_order"], r["count_ms"]["median"], r["trace_plain_ms"]["median"],
                  r["trace_list_ms"]["median"], r["extract_ms"]["median"], r["order_host_ms"]), file=sys.stderr, flush=True)
        print(json.dumps(r), flush=True)
        dev.sync()
        for p in [d_l] + arrays:
            dev.free(p)
    dev.sync()
    for p in (d_dir, d_kind, d_acc, d_w):
        dev.free(p)
    dev.close()


if __name__ == "__main__":
    main()
