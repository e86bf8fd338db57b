#!/usr/bin/env python
"""Frame times of the heightfield ray caster on a 4096 x 4096 scene of TerrainWorld (the full-size
test1_nobn_bilin_both generators, seeded weights): 1920 x 1080 frames at a grazing and at a 45 degree view, the accelerated
march against the plain one (alternated in one process), shadows on against off, and what building the scene costs.

    python tools/render_bench.py [--size 4096] [--dtype bf16x3] [--frame 1080x1920] [--runs 2] [--tiles] [--synthetic]

Prints one JSON line.  Frame times are device-event times around Scene.render (one launch and the download) after a warm-up
frame; each figure is listed once per run, so the spread is visible.  --tiles repeats the accelerated frames with the wave
owning 16 x 4 and 4 x 16 pixels instead of 8 x 8.  --synthetic renders sinusoid terrain instead (no model, no world)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(dev, fn):
    dev.timer_start(0)
    t0 = time.perf_counter()
    out = fn()
    wall = time.perf_counter() - t0
    dev.timer_stop(0)
    return out, dev.timer_ms(0), wall * 1e3


def synthetic(size):
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    hm = np.zeros((size, size), np.float32)
    for i in range(12):
        fy, fx = rng.uniform(-0.02, 0.02, 2) * (1 + i)
        hm += np.float32(rng.uniform(0.3, 1.0) / (1 + i)) * np.sin(np.float32(fy) * yy + np.float32(fx) * xx)
    hm = (hm - hm.min()) / (hm.max() - hm.min())
    return hm[None], rng.uniform(-1, 1, (3, size, size)).astype(np.float32)


def run(a):
    from gan_heightmaps_amd import render as RN
    from gan_heightmaps_amd._lib import tuning_env
    size = a.size
    res = {"size": size, "frame": "%dx%d" % a.frame}
    if a.synthetic:
        from gan_heightmaps_amd.device import Device
        dev, model, world = Device(0), None, None
        hm, tex = synthetic(size)
        vr = (True, False)
    else:
        from gan_heightmaps_amd.experiments import make_model
        model = make_model('test1_nobn_bilin_both', seed=0, verbose=False, use_graph=False, dtype=a.dtype)
        dev = model.device
        world = model.terrain_world(42, overlap=128, batch_size=4)
        world.both(0, 0, world.chunk_px, world.chunk_px)                     # warm-up: builds the plans
        world.clear()
        region = (-size // 2 + 37, -size // 2 - 101, size, size)
        (hm, tex), ms, wall = timed(dev, lambda: world.both(*region))
        res["scene_both"] = {"ms": round(ms, 2), "wall_ms": round(wall, 2)}
        vr = (model.is_a_grayscale, model.is_b_grayscale)
    # the scene's own cost: the host map to [0, 1] and the upload, then the pyramid
    t0 = time.perf_counter()
    scene = RN.Scene(hm, tex, height_scale=a.height_scale, value_range=vr, device=dev)
    dev.sync()
    res["scene_map_upload_pyramid_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    mip, ms, _ = timed(dev, lambda: scene.ops.render_maxmip(scene._hm, size, size))
    res["pyramid_ms"] = round(ms, 3)
    dev.sync()
    dev.free(mip.ptr)
    up = dev.alloc(hm[0].nbytes * 4)
    flat = np.ascontiguousarray(np.concatenate([hm[:1], np.broadcast_to(tex, (3,) + tex.shape[1:])]), np.float32)
    _, ms, _ = timed(dev, lambda: dev.h2d(up, flat))
    res["upload_ms"] = round(ms, 2)
    dev.free(up)

    c = size / 2.0
    views = {"grazing": RN.Camera((c - 0.45 * size, c, a.height_scale * 1.2), 0.0, math.radians(-4.0), size=a.frame),
             "deg45": RN.Camera((c - 0.25 * size, c + 0.1 * size, 0.3 * size), 0.1, math.radians(-45.0), size=a.frame)}
    out = np.empty(a.frame + (3,), np.uint8)
    frames = {}
    for name, cam in views.items():
        f = {}
        scene.render(cam, out=out)                                            # warm-up frame
        ref = None
        for shadows in (True, False):
            key = "shadows" if shadows else "no_shadows"
            f[key] = {"accel_ms": [], "plain_ms": []}
            for _ in range(a.runs):                                           # alternated in one process
                for accel in (True, False):
                    img, ms, _ = timed(dev, lambda: scene.render(cam, out=out, shadows=shadows, accel=accel))
                    f[key]["accel_ms" if accel else "plain_ms"].append(round(ms, 3))
                    if accel:
                        ref = img.copy()
                    else:
                        f[key]["identical"] = bool(np.array_equal(ref, img))
            f[key]["speedup"] = round(min(f[key]["plain_ms"]) / min(f[key]["accel_ms"]), 3)
        depth = np.empty(a.frame, np.float32)
        scene.render(cam, out=out, depth=depth)
        f["sky_share"] = round(float(np.isinf(depth).mean()), 3)
        if a.tiles:
            for tile in ("16x4", "4x16", "8x8"):
                with tuning_env(GHM_RENDER_TILE=tile):
                    scene.render(cam, out=out)
                    f["tile_" + tile + "_ms"] = [round(timed(dev, lambda: scene.render(cam, out=out))[1], 3)
                                                 for _ in range(a.runs)]
        frames[name] = f
    res["frames"] = frames
    if a.save:
        from gan_heightmaps_amd.terrain import _save_png
        for name, cam in views.items():
            _save_png(os.path.join(a.save, "render_bench_%s.png" % name), scene.render(cam))
    scene.close()
    if world is not None:
        world.close()
        model.device.close()
    else:
        dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--frame", default=(1080, 1920), type=lambda s: tuple(int(v) for v in s.lower().split("x")))
    ap.add_argument("--height-scale", type=float, default=256.0)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--tiles", action="store_true", help="also time the other wave tile shapes")
    ap.add_argument("--synthetic", action="store_true", help="sinusoid terrain and noise instead of the world")
    ap.add_argument("--save", default=None, help="directory to write the two views to as PNG")
    a = ap.parse_args()
    print(json.dumps({"tool": "render_bench", "dtype": a.dtype, "results": run(a)}), flush=True)


if __name__ == "__main__":
    main()
