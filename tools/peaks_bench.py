#!/usr/bin/env python
"""Cost of the peaks: what the ascent, the labels, the count, the tree in both forms, the extraction and the host's
merge take, and how many summits there are to rank.

    python tools/peaks_bench.py [--size 4096] [--forms plain,list] [--octaves 8] [--rounds 3] [--height-scale 64]

On one size x size plane of seeded value noise (tools/hydrology_bench.py's): the quantisation once, then per form the ascent, the
labels and areas (ghm_hydrology_accumulate over the ascent), the count, the tree, and the extraction, each between device events
after one warm-up call; a time is the median of ``rounds`` calls.  The labels, the count and the tree wait for the stream
themselves (they return totals), so their times hold that wait; the extraction is followed by a sync inside its window.  A tree
uses up the count's edge offsets, so every tree call is preceded by a count outside its window.  The merge is timed on the host
clock.  peaks.DEFAULT_FORM is the form whose tree was the faster here.

Prints one JSON line per form."""
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
    ap.add_argument("--forms", default="plain,list")
    ap.add_argument("--octaves", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height-scale", type=float, default=64.0)
    a = ap.parse_args()
    from gan_heightmaps_amd import peaks as PK
    from gan_heightmaps_amd.device import Device, Ops
    n = a.size
    cells = n * n
    dev = Device(0)
    ops = Ops(dev)
    h = np.ascontiguousarray(noise_terrain(1, n, a.octaves), np.float32)
    d_h, d_z, d_area, d_label, d_m = (dev.alloc(4 * cells) for _ in range(5))
    d_dir = dev.alloc(cells)
    d_hw, d_w = dev.alloc(ops.hydrology_workspace(n, n)), dev.alloc(ops.peaks_workspace(n, n))
    dev.h2d(d_h, h)

    def window(fn):
        dev.sync()
        dev.timer_start(0)
        fn()
        dev.timer_stop(0)
        return dev.timer_ms(0)                                           # waits for the stop event

    got = {}
    quantise = lambda: ops.viewshed_quantise(d_h, n, n, n, a.height_scale, d_z, n)          # noqa: E731
    ascent = lambda: ops.peaks_ascent(d_z, n, n, n, d_dir, n)                               # noqa: E731

    def labels():
        got["label_rounds"] = ops.hydrology_accumulate(d_dir, n, n, n, d_area, n, d_label, n, d_hw)

    def count():
        got["P"], got["E"] = ops.peaks_count(d_z, n, d_label, n, n, n, d_w)

    for fn in (quantise, ascent, labels, count):
        window(fn)
    P, E = got["P"], got["E"]
    shared = {"tool": "peaks_bench", "size": n, "octaves": a.octaves, "rounds": a.rounds, "height_scale": a.height_scale,
              "summits": P, "edges": E, "label_rounds": got["label_rounds"], "workspace_bytes": ops.peaks_workspace(n, n),
              "list_bytes": ops.peaks_list_bytes(E)}
    for name, fn in (("quantise_ms", quantise), ("ascent_ms", ascent), ("labels_ms", labels), ("count_ms", count)):
        shared[name] = stats([window(fn) for _ in range(a.rounds)])
    zq = np.empty((n, n), np.int32)
    dev.d2h(zq, d_z, zq.nbytes)
    z = zq.ravel()
    arrays = [dev.alloc(max(b, 16)) for b in (4 * P, 4 * P, 12 * (P - 1))]
    host = (np.empty(P, np.int32), np.empty(P, np.uint32), np.empty((P - 1, 3), np.int32))
    for form in a.forms.split(","):
        d_l = dev.alloc(ops.peaks_list_bytes(E)) if form == "list" else None

        def tree():
            got["tree_rounds"] = ops.peaks_tree(d_z, n, d_label, n, n, n, PK.FORMS.index(form), d_m, n, d_w, d_l, P, E)

        def extract():
            ops.peaks_extract(d_label, n, d_area, n, d_m, n, n, n, d_w, P, *arrays)
            dev.sync()

        times = []
        for _ in range(a.rounds + 1):                                    # the first is the warm-up
            count()
            times.append(window(tree))
        r = dict(shared, form=form, tree_rounds=got["tree_rounds"], tree_ms=stats(times[1:]))
        window(extract)
        r["extract_ms"] = stats([window(extract) for _ in range(a.rounds)])
        for x, p in zip(host, arrays):
            if x.nbytes:
                dev.d2h(x, p, x.nbytes)
        t0 = time.perf_counter()
        col, parent, prom = ops.peaks_merge(host[0], z[host[0]], host[2], z[host[2][:, 0]], int(z.min()))
        r["merge_host_ms"] = (time.perf_counter() - t0) * 1e3
        r["reported_at_default"] = int((prom >= PK.Prominence().min_q).sum())
        print("peaks_bench: %s: %d summits, %d edges, %d rounds: ascent %.3f, labels %.3f, count %.3f, tree %.3f, extract %.3f, "
              "merge (host) %.3f ms" % (form, P, E, r["tree_rounds"], r["ascent_ms"]["median"], r["labels_ms"]["median"],
                                        r["count_ms"]["median"], r["tree_ms"]["median"], r["extract_ms"]["median"], r["merge_host_ms"]),
              file=sys.stderr, flush=True)
        print(json.dumps(r), flush=True)
        dev.sync()
        if d_l is not None:
            dev.free(d_l)
    dev.sync()
    for p in [d_h, d_z, d_area, d_label, d_m, d_dir, d_hw, d_w] + arrays:
        dev.free(p)
    dev.close()


if __name__ == "__main__":
    main()
