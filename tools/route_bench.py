#!/usr/bin/env python
"""Cost of the least-cost travel field: which form of the relaxation is faster, and what the other phases cost.

    python tools/route_bench.py [--sizes 1024,4096] [--sources 1,64] [--octaves 8] [--rounds 2]

Per size, on one size x size plane of seeded value noise (tools/hydrology_bench.py's), and per number of sources (seeded cells):
the weights launch, the relaxation in the plain and the tiled form, alternated in one process (plain, tiled, plain, tiled, ...)
after one warm-up call of each, then the parents launch and the hydrology's accumulation over the parent plane; device events
around every call (the relaxation and the accumulation wait for their device word themselves, so a call's time includes those
round trips, as a user pays them).  With each time go the sweeps (launches) or rounds the call ran.  The planes of the two forms
are compared.  The faster form at 4096 is what route.DEFAULT_TILED should say.

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


def bench_size(dev, ops, travel, n, counts, octaves, rounds):
    h = noise_terrain(1, n, octaves)
    cells = n * n
    sizes = (4 * cells, 4 * cells, cells, 4 * cells, 4 * cells, ops.route_workspace(n, n), ops.hydrology_workspace(n, n))
    bufs = [dev.alloc(b) for b in sizes]
    d_h, d_c, d_p, d_a, d_b, ws, hws = bufs
    dev.h2d(d_h, h)

    def timed(fn):
        dev.sync()
        dev.timer_start(0)
        r = fn()
        dev.timer_stop(0)
        return dev.timer_ms(0), r                                        # waits for the stop event

    def weights():
        ops.route_weights(d_h, n, n, n, travel.height_scale, travel.grade, travel.lake, travel.ford, travel.river_threshold,
                          travel.lake_min_depth, ws)

    res = {"size": n}
    timed(weights)
    res["weights_ms"] = stats([timed(weights)[0] for _ in range(rounds)])
    res["sources"] = []
    for count in counts:
        rs = np.random.RandomState(100 + count)
        flat = (rs.randint(0, n, count).astype(np.int64) * n + rs.randint(0, n, count)).tolist()
        times, launches, planes = {False: [], True: []}, {False: [], True: []}, {}
        relax = lambda tiled: ops.route_relax(n, n, flat, tiled, d_c, n, ws)[0]      # noqa: E731
        for tiled in (False, True):                                      # warm-up: code objects loaded, clocks up
            timed(lambda: relax(tiled))
            planes[tiled] = np.empty((n, n), np.uint32)
            dev.d2h(planes[tiled], d_c, planes[tiled].nbytes)
        for _ in range(rounds):
            for tiled in (False, True):
                ms, count_ = timed(lambda: relax(tiled))
                times[tiled].append(ms)
                launches[tiled].append(count_)
        r = {"sources": count, "plain_ms": stats(times[False]), "tiled_ms": stats(times[True]), "plain_sweeps": launches[False],
             "tiled_launches": launches[True], "bit_identical": bool(planes[False].tobytes() == planes[True].tobytes())}
        r["plain_over_tiled"] = round(r["plain_ms"]["median"] / r["tiled_ms"]["median"], 3)
        r["faster"] = "tiled" if r["tiled_ms"]["median"] < r["plain_ms"]["median"] else "plain"
        reached = planes[True] != 0xFFFFFFFF
        r["reached_cells"] = int(reached.sum())
        r["largest_cost_units"] = int(planes[True][reached].max())
        parents = lambda: ops.route_parents(d_c, n, n, n, d_p, n, ws)     # noqa: E731
        timed(parents)
        r["parents_ms"] = stats([timed(parents)[0] for _ in range(rounds)])
        acc = lambda: ops.hydrology_accumulate(d_p, n, n, n, d_a, n, d_b, n, hws)      # noqa: E731
        timed(acc)
        runs = [timed(acc) for _ in range(rounds)]
        r["accumulate_ms"] = stats([x[0] for x in runs])
        r["accumulate_rounds"] = runs[0][1]
        A = np.empty((n, n), np.uint32)
        dev.d2h(A, d_a, A.nbytes)
        r["traffic_at_sources_is_reached_cells"] = bool(int(A.ravel()[sorted(set(flat))].astype(np.int64).sum()) == r["reached_cells"])
        res["sources"].append(r)
    dev.sync()
    for p in bufs:
        dev.free(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--sources", default="1,64")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    from gan_heightmaps_amd import route as RT
    from gan_heightmaps_amd.device import Device, Ops
    dev = Device(0)
    ops = Ops(dev)
    counts = [int(s) for s in a.sources.split(",")]
    out = {"tool": "route_bench", "octaves": a.octaves, "rounds": a.rounds, "tile": 32, "inner_sweeps": 32,
           "default_tiled": RT.DEFAULT_TILED, "planes": [bench_size(dev, ops, RT.Travel(), int(s), counts, a.octaves, a.rounds)
                                                        for s in a.sizes.split(",")]}
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
