#!/usr/bin/env python
"""What a render scene of TerrainWorld costs to build through the host and on the device, and what a flight makes of it
(DESIGN §4n).  The full-size test1_nobn_bilin_both generators with seeded weights, one process, one MI355X.

    python tools/flight_bench.py [--size 4096] [--dtype bf16x3] [--runs 2] [--frames 300] [--frame 270x480]
        [--path-px 6000] [--max-dist 600] [--window-mb 96]

Prints one JSON line.
  scene_build: the same size x size rectangle built as scene() and as scene(resident=True), alternated, ``runs`` times, once
      from an empty chunk cache ("cold": the chunks are computed too) and once with the chunks resident ("warm": texture,
      sinks and pyramid only).  Wall-clock milliseconds from the call to the synchronised device.  The host path is split
      into ``both`` (chunks + texture + download) and the Scene constructor (the map to [0, 1], the upload and the pyramid);
      the pyramid's own device-event time is listed once, it is the same kernel on both paths.  cold - warm is the chunks' share.
  flight: frames per second of a straight path of ``frames`` frames through several windows, and the share of the wall time
      spent building windows (the calls to scene(resident=True) inside flight)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(dev, fn):
    dev.sync()
    t0 = time.perf_counter()
    out = fn()
    dev.sync()
    return out, (time.perf_counter() - t0) * 1e3


def build_host(world, model, region, hs):
    from gan_heightmaps_amd import render as RN
    dev = model.device
    (hm, tex), t_both = wall_ms(dev, lambda: world.both(*region))
    scene, t_ctor = wall_ms(dev, lambda: RN.Scene(hm, tex, origin=region[:2], height_scale=hs, device=dev,
                                                  value_range=(model.is_a_grayscale, model.is_b_grayscale)))
    return scene, {"both_ms": round(t_both, 1), "map_upload_pyramid_ms": round(t_ctor, 1), "total_ms": round(t_both + t_ctor, 1)}


def build_resident(world, model, region, hs):
    scene, t = wall_ms(model.device, lambda: world.scene(*region, resident=True, height_scale=hs))
    return scene, {"total_ms": round(t, 1)}


def run(a):
    from gan_heightmaps_amd import render as RN
    from gan_heightmaps_amd.experiments import make_model
    model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=a.dtype)
    dev = model.device
    world = model.terrain_world(42, overlap=128, batch_size=4)
    K = world.chunk_px
    world.both(0, 0, K // 4, K // 4)                                          # warm-up: plans, kernels
    world.scene(0, 0, K // 4, K // 4, resident=True).close()
    world.clear()
    size, hs = a.size, a.height_scale
    region = (-size // 2 + 37, -size // 2 - 101, size, size)
    res = {"size": size, "region": list(region), "chunk_px": K, "runs": []}
    cam = RN.Camera((region[0] + 0.25 * size, region[1] + 0.6 * size, 0.3 * size), 0.1, -0.785, size=(270, 480))
    for _ in range(a.runs):
        r = {}
        for cache in ("cold", "warm"):
            imgs = {}
            for path, build in (("host", build_host), ("resident", build_resident)):      # alternated in one process
                if cache == "cold":
                    world.clear()
                scene, r[path + "_" + cache] = build(world, model, region, hs)
                imgs[path] = scene.render(cam)
                if "pyramid_event_ms" not in res:
                    dev.timer_start(0)
                    mip = scene.ops.render_maxmip(scene._hm, size, size)
                    dev.timer_stop(0)
                    res["pyramid_event_ms"] = round(dev.timer_ms(0), 3)
                    dev.sync()
                    dev.free(mip.ptr)
                scene.close()
            r["identical_" + cache] = bool(np.array_equal(imgs["host"], imgs["resident"]))
        res["runs"].append(r)
    best = lambda k: min(x[k]["total_ms"] for x in res["runs"])
    res["best_total_ms"] = {k: best(k) for k in ("host_cold", "resident_cold", "host_warm", "resident_warm")}
    res["resident_over_host"] = {c: round(best("resident_" + c) / best("host_" + c), 3) for c in ("cold", "warm")}

    # ---- a flight: a straight path through several windows ----
    world.clear()
    n = a.frames
    cams = [RN.Camera((-a.path_px / 2.0 + a.path_px * i / (n - 1.0), 300.25, 0.5 * a.max_dist), 0.1, -0.6, size=a.frame)
            for i in range(n)]
    plan = world.flight_plan(cams, a.max_dist, window_mb=a.window_mb)
    builds, inner = [], world.scene

    def timed_scene(*args, **kw):
        sc, t = wall_ms(dev, lambda: inner(*args, **kw))
        builds.append(t)
        return sc
    world.scene = timed_scene                                                 # flight builds its windows through self.scene
    out = np.empty(a.frame + (3,), np.uint8)
    before = world.computed
    _, total = wall_ms(dev, lambda: sum(1 for _ in world.flight(cams, a.max_dist, window_mb=a.window_mb, height_scale=hs,
                                                                out=out)))
    del world.scene
    res["flight"] = {"frames": n, "frame": "%dx%d" % a.frame, "path_px": a.path_px, "max_dist": a.max_dist,
                     "window_mb": a.window_mb, "windows": len(plan),
                     "window_px": ["%dx%d" % (r[2], r[3]) for r, _, _ in plan],
                     "frames_per_window": [j - i + 1 for _, i, j in plan], "chunks_computed": world.computed - before,
                     "wall_ms": round(total, 1), "fps": round(n / (total / 1e3), 2),
                     "window_build_ms": [round(t, 1) for t in builds],
                     "build_share": round(sum(builds) / total, 3),
                     "fps_rendering_alone": round(n / ((total - sum(builds)) / 1e3), 2)}
    world.close()
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--height-scale", type=float, default=256.0)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--frame", default=(270, 480), type=lambda s: tuple(int(v) for v in s.lower().split("x")))
    ap.add_argument("--path-px", type=float, default=6000.0)
    ap.add_argument("--max-dist", type=float, default=600.0)
    ap.add_argument("--window-mb", type=float, default=96.0)
    a = ap.parse_args()
    print(json.dumps({"tool": "flight_bench", "dtype": a.dtype, "results": run(a)}), flush=True)


if __name__ == "__main__":
    main()
