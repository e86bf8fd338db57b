#!/usr/bin/env python
"""Cost of the adaptive mesh: which of the two forms of ghm_mesh_errors is faster, and what a cut costs.

    python tools/mesh_bench.py [--size 4097] [--tile 256] [--rounds 2] [--repeat 5]

The plain and the fused form of the error map on one size x size plane of a seeded sine terrain, alternated in one process
(plain, fused, plain, fused, ...) after one warm-up call of each; device events around ``repeat`` calls per window.  Then
ghm_mesh_count and ghm_mesh_extract (the device work and the wait for the totals; no allocation, no download) at three
tolerances taken from the error plane's quantiles, so that about 1 %, 10 % and 50 % of the vertices survive: V, F, the
share of the full triangulation and the triangles per second.  The faster form is what mesh.DEFAULT_FUSED should say.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.skylight_bench import sine_terrain  # noqa: E402


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4), "runs": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4097)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    from gan_heightmaps_amd import mesh as MS
    from gan_heightmaps_amd.device import Device, Ops
    n, k = a.size, MS._tile_log2(a.tile)
    if (n - 1) % a.tile or n <= a.tile:
        raise SystemExit("--size must be R tile + 1")
    dev = Device(0)
    ops = Ops(dev)
    src, err = dev.alloc(4 * n * n), dev.alloc(4 * n * n)
    dev.h2d(src, sine_terrain(1, n))

    def timed(fn, repeat):
        dev.sync()
        dev.timer_start(0)
        for _ in range(repeat):
            fn()
        dev.timer_stop(0)
        return dev.timer_ms(0) / repeat                    # waits for the stop event

    def errors(fused):
        ops.mesh_errors(src, n, n, n, k, fused, err, n)

    times, planes = {False: [], True: []}, {}
    for fused in (False, True):                            # warm-up: code objects loaded, clocks up
        timed(lambda: errors(fused), 1)
    for _ in range(a.rounds):
        for fused in (False, True):
            times[fused].append(timed(lambda: errors(fused), a.repeat))
    for fused in (False, True):
        dev.memset_zero(err, 4 * n * n)
        timed(lambda: errors(fused), 1)
        planes[fused] = np.empty((n, n), np.float32)
        dev.d2h(planes[fused], err, planes[fused].nbytes)
    e = planes[True]
    finite = e[np.isfinite(e)]
    full = 2 * (n - 1) * (n - 1)
    ws = dev.alloc(ops.mesh_workspace(n - 1, n - 1))
    index = dev.alloc(4 * n * n)
    cuts = []
    for share in (0.01, 0.1, 0.5):
        tol = float(np.quantile(finite, 1.0 - share))
        V, F = ops.mesh_count(err, n, n, n, k, 0, 0, n - 1, n - 1, tol, ws)          # warm-up, and the sizes
        bufs = [dev.alloc(max(4, b)) for b in (8 * V, 4 * V, 12 * F)]
        extract = lambda: ops.mesh_extract(src, n, err, n, n, n, k, 0, 0, n - 1, n - 1, tol, ws, index, *bufs, V, F)  # noqa: E731
        extract()
        t_count = [timed(lambda: ops.mesh_count(err, n, n, n, k, 0, 0, n - 1, n - 1, tol, ws), a.repeat) for _ in range(a.rounds)]
        t_extract = [timed(extract, a.repeat) for _ in range(a.rounds)]
        dev.sync()
        for p in bufs:
            dev.free(p)
        cuts.append({"vertex_share": share, "max_error": tol, "V": V, "F": F, "share_of_full": round(F / full, 4),
                     "count_ms": stats(t_count), "extract_ms": stats(t_extract),
                     "mtriangles_per_s": round(F / stats(t_extract)["median"] / 1e3, 1)})
    res = {"tool": "mesh_bench", "size": n, "tile": a.tile, "rounds": a.rounds, "repeat": a.repeat,
           "fused_levels": 3, "plain_ms": stats(times[False]), "fused_ms": stats(times[True]),
           "floor_bytes": 8 * n * n, "bit_identical": bool(planes[False].tobytes() == planes[True].tobytes()), "cuts": cuts}
    res["plain_gb_per_s_of_floor"] = round(8 * n * n / res["plain_ms"]["median"] / 1e6, 1)
    res["fused_gb_per_s_of_floor"] = round(8 * n * n / res["fused_ms"]["median"] / 1e6, 1)
    res["plain_over_fused"] = round(res["plain_ms"]["median"] / res["fused_ms"]["median"], 3)
    res["faster"] = "fused" if res["plain_over_fused"] > 1 else "plain"
    dev.sync()
    for p in (src, err, ws, index):
        dev.free(p)
    dev.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
