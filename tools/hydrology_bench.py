#!/usr/bin/env python
"""Cost of the hydrology: which form of the two relaxations is faster, and what the other phases cost.

    python tools/hydrology_bench.py [--sizes 1024,4096] [--octaves 8] [--rounds 2]

Per size, on one size x size plane of seeded value noise: the filled surface and the flat distance in the plain and the tiled
form, alternated in one process (plain, tiled, plain, tiled, ...) after one warm-up call of each, then the direction launch and
the accumulation; device events around every call (the entry points of the relaxations and of the accumulation wait for their
device word themselves, so a call's time includes those round trips, as a user pays them).  With each time go the sweeps
(launches) or rounds the call ran.  The planes of the two forms are compared.  The faster form at 4096 is what
hydrology.DEFAULT_TILED should say.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def noise_terrain(seed, n, octaves):
    """``octaves`` octaves of bilinearly interpolated value noise on an n x n plane, normalised to [0, 1], float32"""
    rs = np.random.RandomState(seed)
    t = np.zeros((n, n), np.float32)
    for o in range(octaves):
        m = 2 << o
        g = rs.rand(m + 1, m + 1).astype(np.float32)
        p = np.arange(n, dtype=np.float64) * m / n
        i = np.floor(p).astype(np.int64)
        f = (p - i).astype(np.float32)
        rows = g[i] + f[:, None] * (g[i + 1] - g[i])                    # [n, m + 1]
        t += (rows[:, i] + f[None, :] * (rows[:, i + 1] - rows[:, i])) * np.float32(0.5 ** o)
    t -= t.min()
    t /= t.max()
    return np.ascontiguousarray(t)


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4), "runs": [round(x, 4) for x in v]}


def bench_size(dev, ops, n, octaves, rounds):
    h = noise_terrain(1, n, octaves)
    cells = n * n
    sizes = (4 * cells, 4 * cells, 4 * cells, cells, 4 * cells, 4 * cells, ops.hydrology_workspace(n, n))
    bufs = [dev.alloc(b) for b in sizes]
    d_h, d_f, d_d, d_dir, d_a, d_b, ws = bufs
    dev.h2d(d_h, h)

    def timed(fn):
        dev.sync()
        dev.timer_start(0)
        r = fn()
        dev.timer_stop(0)
        return dev.timer_ms(0), r                                        # waits for the stop event

    def fill(tiled):
        return ops.hydrology_fill(d_h, n, n, n, tiled, d_f, n, ws)[0]

    def flats(tiled):
        return ops.hydrology_flats(d_f, n, n, n, tiled, d_d, n, ws)

    res = {"size": n}
    for name, fn, ptr, dtype in (("fill", fill, d_f, np.float32), ("flats", flats, d_d, np.int32)):
        times, counts, planes = {False: [], True: []}, {False: [], True: []}, {}
        for tiled in (False, True):                                      # warm-up: code objects loaded, clocks up
            timed(lambda: fn(tiled))
            planes[tiled] = np.empty((n, n), dtype)
            dev.d2h(planes[tiled], ptr, planes[tiled].nbytes)
        for _ in range(rounds):
            for tiled in (False, True):
                ms, count = timed(lambda: fn(tiled))
                times[tiled].append(ms)
                counts[tiled].append(count)
        res[name] = {"plain_ms": stats(times[False]), "tiled_ms": stats(times[True]), "plain_sweeps": counts[False],
                     "tiled_launches": counts[True], "bit_identical": bool(planes[False].tobytes() == planes[True].tobytes())}
        res[name]["plain_over_tiled"] = round(res[name]["plain_ms"]["median"] / res[name]["tiled_ms"]["median"], 3)
        if name == "fill":
            res["lake_cells"] = int((planes[True] > h).sum())
        else:
            res["non_draining_cells"] = int((planes[True] > 0).sum())
            res["largest_flat_distance"] = int(planes[True].max())
    timed(lambda: ops.hydrology_directions(d_f, n, d_d, n, n, n, d_dir, n))
    res["directions_ms"] = stats([timed(lambda: ops.hydrology_directions(d_f, n, d_d, n, n, n, d_dir, n))[0]
                                  for _ in range(rounds)])
    acc = lambda: ops.hydrology_accumulate(d_dir, n, n, n, d_a, n, d_b, n, ws)      # noqa: E731
    timed(acc)
    runs = [timed(acc) for _ in range(rounds)]
    res["accumulate_ms"] = stats([r[0] for r in runs])
    res["accumulate_rounds"] = runs[0][1]
    A = np.empty((n, n), np.uint32)
    dev.d2h(A, d_a, A.nbytes)
    edge = np.concatenate([A[0], A[-1], A[1:-1, 0], A[1:-1, -1]]).astype(np.int64)
    res["outlets_sum_to_cells"] = bool(edge.sum() == cells)
    res["largest_area"] = int(A.max())
    plain = res["fill"]["plain_ms"]["median"] + res["flats"]["plain_ms"]["median"]
    tiled = res["fill"]["tiled_ms"]["median"] + res["flats"]["tiled_ms"]["median"]
    res["relaxations_plain_ms"], res["relaxations_tiled_ms"] = round(plain, 4), round(tiled, 4)
    res["faster"] = "tiled" if tiled < plain else "plain"
    dev.sync()
    for p in bufs:
        dev.free(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    from gan_heightmaps_amd import hydrology as HY
    from gan_heightmaps_amd.device import Device, Ops
    dev = Device(0)
    ops = Ops(dev)
    out = {"tool": "hydrology_bench", "octaves": a.octaves, "rounds": a.rounds, "tile": 32, "inner_sweeps": 32,
           "default_tiled": HY.DEFAULT_TILED, "planes": [bench_size(dev, ops, int(s), a.octaves, a.rounds)
                                                        for s in a.sizes.split(",")]}
    dev.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
