#!/usr/bin/env python
"""Cost of the sliced Wasserstein distance's kernels at the sizes of the default ``Pix2Pix.swd`` call: 1024
images of 512 x 512 in batches of 4, 128 windows per image (N = 2^17 descriptors per level), 128 directions per repeat.

    python tools/swd_bench.py [--channels 1 3] [--rounds 5] [--chunks 32768 4096 1024]

Per channel count, device events around each stage after one warm-up call, ``rounds`` timed calls, median / min / max in ms:
  pyramid      one batch of 4 images through all six levels (ghm_swd_pyramid_level x 6)
  gather       the same batch's windows of all six levels (ghm_swd_gather x 6)
  stats        one level's [N, 49 C] matrix
  project      one level, one repeat: [N, 49 C] x [49 C, 128] -> [128, N]
  sort_lds     512 columns of 2^15 floats: the one-workgroup form, the same number of floats as a repeat's projection
  sort_global  128 columns of 2^17 floats: the global form, per LDS chunk size of --chunks
  l1           two [128, N] buffers
and ``call_estimate_ms``: what the stages add up to for one net's whole comparison (256 batches and 6 levels x 4 repeats x
2 sets).  Every sort's result is checked to be ascending and a permutation (its sum) before its time counts.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(dev, fn):
    dev.timer_start(0)
    fn()
    dev.timer_stop(0)
    return dev.timer_ms(0)                                # waits for the stop event


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def bench(C, rounds, chunks):
    from gan_heightmaps_amd import swd as SW
    from gan_heightmaps_amd.device import Device, DevTensor, Ops
    dev = Device(0)
    ops = Ops(dev)
    metric = SW.SWD()
    B, S, n_img, D = 4, 512, 1024, metric.directions
    N, K = n_img * metric.patches_per_image, 49 * C
    rs = np.random.RandomState(C)
    res = {"C": C, "N": N, "K": K, "directions": D}

    def measure(fn, setup=None):
        out = []
        for r in range(rounds + 1):
            if setup is not None:
                setup()
            dev.sync()
            ms = timed(dev, fn)
            if r:
                out.append(ms)
        return spread(out)

    with SW.Descriptors(ops, metric, 0, n_img, C, S, S, max_batch=B) as d:
        batch = dev.tensor(rs.uniform(-1, 1, (B, C, S, S)).astype(np.float32))
        laps = [dev.alloc(4 * B * C * h * w) for h, w in d.sizes]

        def pyramid():
            g = batch
            for i, (h, w) in enumerate(d.sizes):
                nxt = d._g[i % 2] if i < d.L - 1 else None
                ops.swd_pyramid_level(g, None, nxt, w // 2, laps[i], w)
                if nxt is not None:
                    g = DevTensor(dev, nxt, (B, C, h // 2, w // 2))

        def gather():
            for i, (h, w) in enumerate(d.sizes):
                ops.swd_gather(laps[i], B, C, h, w, w, d._corners[i], d.P, d.desc[i], 0, N)

        res["pyramid"], res["gather"] = measure(pyramid), measure(gather)
        for p in laps + [batch.ptr]:
            dev.free(p)
        # one level's matrix: unit normal values with a shift per channel
        x = (rs.randn(N, C, 49) + np.arange(C)[None, :, None]).astype(np.float32)
        dev.h2d(d.desc[0], x)
        ws, st, dirs = dev.alloc(ops.swd_workspace()), dev.alloc(8 * C), dev.alloc(4 * K * D)
        pa, pb = dev.alloc(4 * D * N), dev.alloc(4 * D * N)
        dev.h2d(dirs, SW.directions(metric, 0, 0, K))
        res["stats"] = measure(lambda: ops.swd_stats(d.desc[0], N, C, st, ws))
        res["project"] = measure(lambda: ops.swd_project(d.desc[0], N, C, dirs, D, st, pa))
        dev.sync()
        proj = np.empty((D, N), np.float32)
        dev.d2h(proj, pa, proj.nbytes)
        want = (((x.astype(np.float64) - x.mean(axis=(0, 2), keepdims=True)) / x.std(axis=(0, 2), keepdims=True))
                .reshape(N, K)[:4096] @ SW.directions(metric, 0, 0, K).astype(np.float64)).T
        res["project_max_error"] = float(np.abs(proj[:, :4096] - want).max())

        def check_sorted(n_cols, n):
            dev.sync()
            got = np.empty((n_cols, n), np.float32)
            dev.d2h(got, pb, got.nbytes)
            ok = bool((np.diff(got, axis=1) >= 0).all()) and bool(np.array_equal(np.sort(proj.reshape(n_cols, n), axis=1), got))
            if not ok:
                raise RuntimeError("a sort's result is not numpy.sort's")

        refill = lambda: dev.d2d(pb, pa, 4 * D * N)
        res["sort_lds"] = measure(lambda: ops.swd_sort_columns(pb, 1 << 15, D * N >> 15), refill)
        check_sorted(D * N >> 15, 1 << 15)
        res["sort_global"] = {}
        for chunk in chunks:
            res["sort_global"][str(chunk)] = measure(lambda: ops.swd_sort_columns(pb, N, D, chunk), refill)
            check_sorted(D, N)
        res["l1"] = measure(lambda: ops.swd_l1(pa, pb, D * N, ws))
        for p in (ws, st, dirs, pa, pb):
            dev.free(p)
    med = lambda k: res[k]["median"]
    levels, repeats = 6, metric.repeats
    res["call_estimate_ms"] = round(
        2 * (n_img // B) * (med("pyramid") + med("gather"))
        + levels * (2 * med("stats") + repeats * (2 * (med("project") + res["sort_global"][str(chunks[0])]["median"]) + med("l1"))),
        1)
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", type=int, nargs="+", default=[32768, 4096, 1024])
    a = ap.parse_args()
    print(json.dumps({"tool": "swd_bench", "rounds": a.rounds, "results": [bench(c, a.rounds, a.chunks) for c in a.channels]}),
          flush=True)


if __name__ == "__main__":
    main()
