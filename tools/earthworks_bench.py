#!/usr/bin/env python
"""Cost of the earthworks: which form of the nearest-mark search is faster, and what the shaping costs.

    python tools/earthworks_bench.py [--size 4096] [--reaches 4,32] [--octaves 8] [--rounds 5] [--launches 10]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's) the hydrology is analysed once and the river cells of
earthworks.Channel() are the marks.  Per reach: the nearest mark in the plain and the tiled form, alternated in one process
(plain, tiled, plain, tiled, ...) after one warm-up window of each; a window is ``launches`` launches between two device events
(the plain form at a reach above 8 is given a tenth of them: it is the slow one), a time is a window's over its launches, and
the median of ``rounds`` windows is reported.  The planes of the two forms are compared.  The same on ``dense`` marks, one per
32 x 32 tile, where no tile of the tiled form is empty (``empty_windows`` is the share of the tiles the empty-tile skip fires on;
what the skip is worth shows against a tuning build with GHM_BUILD_DEFINES=-DGHM_EARTHWORKS_NO_SKIP).  Then the
shaping at the channel's profile.  The faster form is what earthworks.DEFAULT_TILED should say.

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


def empty_windows(marks, R, tile=32):
    """the share of the tiles whose (tile + 2R)^2 window holds no mark"""
    n = marks.shape[0]
    c = np.zeros((n + 1, n + 1), np.int64)
    c[1:, 1:] = (marks != 0).cumsum(0).cumsum(1)
    empty = total = 0
    for ty in range(0, n, tile):
        y0, y1 = max(0, ty - R), min(n, ty + tile + R)
        for tx in range(0, n, tile):
            x0, x1 = max(0, tx - R), min(n, tx + tile + R)
            empty += (c[y1, x1] - c[y0, x1] - c[y1, x0] + c[y0, x0]) == 0
            total += 1
    return round(float(empty) / total, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reaches", default="4,32")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    from gan_heightmaps_amd import earthworks as EW
    from gan_heightmaps_amd import hydrology as HY
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    dev = Device(0)
    ops = Ops(dev)
    hydro = HY.analyse(ops, noise_terrain(1, n, a.octaves), keep=('filled', 'depth', 'accumulation'))
    channel = EW.Channel()
    rivers, target = EW.channel_targets(hydro.filled, hydro.depth, hydro.accumulation, channel)
    dense = np.zeros((n, n), np.uint32)
    dense[13::32, 17::32] = 1
    cells = n * n
    bufs = [dev.alloc(4 * cells) for _ in range(6)]
    d_m, d_n, d_d, d_h, d_t, d_o = bufs
    dev.h2d(d_h, hydro.filled)
    dev.h2d(d_t, target)

    def window(fn, launches):
        dev.sync()
        dev.timer_start(0)
        for _ in range(launches):
            fn()
        dev.timer_stop(0)
        return dev.timer_ms(0) / launches                                # waits for the stop event

    out = {"tool": "earthworks_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "launches": a.launches, "tile": 32,
           "default_tiled": EW.DEFAULT_TILED, "river_cells": int(rivers.sum()), "nearest": []}
    for name, marks in (("rivers", rivers), ("dense", dense)):
        dev.h2d(d_m, marks)
        for R in [int(s) for s in a.reaches.split(",")]:
            count = {False: max(1, a.launches // 10) if R > 8 else a.launches, True: a.launches}
            near = lambda tiled: ops.earthworks_nearest(d_m, n, n, n, 1, R, tiled, d_n, n, d_d, n)      # noqa: E731
            times, planes = {False: [], True: []}, {}
            for tiled in (False, True):                                  # warm-up: code objects loaded, clocks up
                window(lambda: near(tiled), count[tiled])
                planes[tiled] = (np.empty((n, n), np.int32), np.empty((n, n), np.int32))
                dev.d2h(planes[tiled][0], d_n, 4 * cells)
                dev.d2h(planes[tiled][1], d_d, 4 * cells)
            for _ in range(a.rounds):
                for tiled in (False, True):
                    times[tiled].append(window(lambda: near(tiled), count[tiled]))
            r = {"marks": name, "reach": R, "plain_ms": stats(times[False]), "tiled_ms": stats(times[True]),
                 "lds_bytes": ops.earthworks_lds_bytes(R), "empty_windows": empty_windows(marks, R),
                 "found_cells": int((planes[True][0] >= 0).sum()),
                 "bit_identical": bool(all(planes[False][i].tobytes() == planes[True][i].tobytes() for i in (0, 1)))}
            r["plain_over_tiled"] = round(r["plain_ms"]["median"] / r["tiled_ms"]["median"], 3)
            r["faster"] = "tiled" if r["tiled_ms"]["median"] < r["plain_ms"]["median"] else "plain"
            out["nearest"].append(r)
    # the shaping, on the river marks at the channel's profile
    prof = channel.profile
    table = prof.table()
    d_tab = dev.alloc(table.nbytes)
    bufs.append(d_tab)
    dev.h2d(d_tab, table)
    dev.h2d(d_m, rivers)
    ops.earthworks_nearest(d_m, n, n, n, 1, prof.R, True, d_n, n, d_d, n)
    shape = lambda: ops.earthworks_shape(d_h, n, d_n, n, d_d, n, d_t, n, d_tab, prof.R, prof.mode_index, n, n, d_o, n)    # noqa: E731
    window(shape, a.launches)
    out["shape_ms"] = stats([window(shape, a.launches) for _ in range(a.rounds)])
    carved = np.empty((n, n), np.float32)
    dev.d2h(carved, d_o, 4 * cells)
    out["cut_volume"] = round(float((hydro.filled.astype(np.float64) - carved).sum()), 3)
    dev.sync()
    for p in bufs:
        dev.free(p)
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
