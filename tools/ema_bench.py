#!/usr/bin/env python
"""What the exponential moving average of the generator weights costs on the MI355X.  One process:

    python tools/ema_bench.py [--reps 50] [--warmup 5] [--steps 40] [--blocks 5] [--out FILE]

(a) ghm_ema_update alone on buffers of the two full-size generators' n_train (experiment test1_nobn_bilin_both), beside
    ghm_opt_update rule 'sgd' at the same n: both read two fp32 buffers and write one (12 bytes per element), so sgd is the
    yardstick.  The two launches alternate, each timed with HIP events ``--reps`` times after ``--warmup`` untimed pairs;
    medians, the effective rate 12 n / time, and the ratio ema / sgd (target: <= 1.10, the margin being the event timers'
    noise on launches this short).
(b) the whole joint train step (bench.py's workload: batch 4, 'bf16x3', recorded issue, one resident batch) of a model with
    ema=None and one with ema=0.999, alternating blocks of ``--steps`` steps, ``--blocks`` blocks each; median ms per step
    of each and the difference.  No threshold: the figure is reported as it is.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENS = ['dcgan_gen', 'p2p_gen']


def kernel_ab(dev, ops, sizes, reps, warmup):
    rng = np.random.RandomState(0)
    rows = []
    for k in GENS:
        n = sizes[k]
        p, w = (dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32) * 0.05) for _ in range(2))
        g = dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32) * 1e-3)
        ema = dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32) * 0.05)
        hyper = dev.tensor(np.array([1e-5, 0.0], np.float32))
        runs = {'sgd': lambda: ops.opt_update('sgd', p, g, [], n, hyper, ()),
                'ema': lambda: ops.ema_update(ema, w, n, 0.999)}
        for _ in range(warmup):
            for run in runs.values():
                run()
        for r in range(reps):               # alternated: slot 2r = sgd, 2r + 1 = ema
            for j, run in enumerate(runs.values()):
                dev.timer_start(2 * r + j)
                run()
                dev.timer_stop(2 * r + j)
        dev.sync()
        ms = {name: [dev.timer_ms(2 * r + j) for r in range(reps)] for j, name in enumerate(runs)}
        row = {'net': k, 'n': n}
        for name, v in ms.items():
            med = float(np.median(v))
            row[name] = {'ms': med, 'ms_min': float(np.min(v)), 'ms_p90': float(np.percentile(v, 90)),
                         'TB_s': 12.0 * n / (med * 1e-3) / 1e12}
        row['ema_over_sgd'] = row['ema']['ms'] / row['sgd']['ms']
        rows.append(row)
        print("%-10s n=%-9d sgd %.4f ms (%.2f TB/s)   ema %.4f ms (%.2f TB/s)   ema / sgd = %.3f  [median of %d, alternated]"
              % (k, n, row['sgd']['ms'], row['sgd']['TB_s'], row['ema']['ms'], row['ema']['TB_s'], row['ema_over_sgd'], reps),
              flush=True)
        for t in (p, w, g, ema, hyper):
            dev.free(t.ptr)
    return rows


def step_ab(dev, steps, blocks):
    from bench import synthetic_batch
    from gan_heightmaps_amd.experiments import make_model
    models = {}
    for name, ema in (('none', None), ('ema', 0.999)):
        m = make_model('test1_nobn_bilin_both', device=dev, use_graph='recorded', seed=0, verbose=False, dtype='bf16x3', ema=ema)
        eng = m.engine
        b = eng.built(4)
        eng._upload(b, *synthetic_batch(4, 1000, 512, seed=1000))
        for _ in range(5):                  # eager, record, warm replays
            eng.enqueue_train(b)
        eng.sync()
        models[name] = (m, eng, b)
    ms = {name: [] for name in models}
    for _ in range(blocks):
        for name, (m, eng, b) in models.items():
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.enqueue_train(b)
            eng.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {name: {'ms_per_step_blocks': v, 'ms_per_step': float(np.median(v))} for name, v in ms.items()}
    res['steps_per_block'], res['blocks'] = steps, blocks
    res['ema_minus_none_ms'] = res['ema']['ms_per_step'] - res['none']['ms_per_step']
    res['relative'] = res['ema_minus_none_ms'] / res['none']['ms_per_step']
    for name in ms:
        print("step ema=%-5s %.3f ms (blocks %s)" % ('None' if name == 'none' else '0.999', res[name]['ms_per_step'],
                                                     ", ".join("%.3f" % v for v in ms[name])), flush=True)
    print("ema - none: %+.3f ms per step (%+.2f %%), %d blocks of %d steps each, alternated"
          % (res['ema_minus_none_ms'], 100 * res['relative'], blocks, steps), flush=True)
    sizes = {k: models['ema'][1].stores[k].n_train for k in GENS}
    return res, sizes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON")
    args = ap.parse_args(argv)
    if not 1 <= args.reps <= 2000:
        sys.exit("ema_bench.py: --reps must be in 1 .. 2000 (two timer slots per repetition)")
    from gan_heightmaps_amd import device
    if device.device_count() == 0:
        sys.exit("ema_bench.py: no HIP device visible")
    dev = device.Device(0)
    ab, sizes = step_ab(dev, args.steps, args.blocks)
    kdev = device.Device(0)                 # a context of its own: the models' recorded steps stay on theirs
    res = {'device': dev.info(), 'reps': args.reps, 'warmup': args.warmup, 'sizes': sizes, 'step_ab': ab,
           'kernels': kernel_ab(kdev, device.Ops(kdev), sizes, args.reps, args.warmup)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
