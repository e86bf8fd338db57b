#!/usr/bin/env python
"""Rate of the nine optimiser kernels on the flat parameter buffers of experiment test1_nobn_bilin_both (MI355X).

    python tools/opt_update_bench.py [--reps 20] [--warmup 3] [--step-ab STEPS] [--out FILE]

For every rule (rmsprop / adam: elementwise.hip; the other seven: ghm_opt_update, optim.hip) and each of the four nets'
flat fp32 buffers, one update launch is timed with HIP events ``--reps`` times after ``--warmup`` untimed launches; the
median is printed with the effective rate = bytes per parameter x n / time (the bytes every rule must move: p read and
written, g read, each state buffer read and written).

``--step-ab STEPS``: the whole joint train step (bench.py's workload: batch 4, 'bf16x3', recorded issue, one resident
batch) with opt=amsgrad against opt=rmsprop: STEPS timed steps per block, the two alternating, each block in a child
process of its own (three blocks each); reports the median ms per step and the difference.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = ['dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc']
# rule -> (fp32 state buffers, hyper-parameters in the order of the launch)
RULES = {
    'sgd': (0, ()),
    'momentum': (1, (0.9,)),
    'nesterov_momentum': (1, (0.9,)),
    'adagrad': (1, (1e-6,)),
    'rmsprop': (1, (0.9, 1e-6)),
    'adadelta': (2, (0.95, 1e-6)),
    'adam': (2, (0.9, 0.999, 1e-8)),
    'adamax': (2, (0.9, 0.999, 1e-8)),
    'amsgrad': (3, (0.9, 0.999, 1e-8)),
}


def bytes_per_param(rule):
    return 12 + 8 * RULES[rule][0]


def launcher(ops, rule, p, g, st, n, hyper):
    h = RULES[rule][1]
    if rule == 'rmsprop':
        return lambda: ops.rmsprop(p, g, st[0], n, hyper, *h)
    if rule == 'adam':
        return lambda: ops.adam(p, g, st[0], st[1], n, hyper, *h)
    return lambda: ops.opt_update(rule, p, g, st, n, hyper, h)


def kernel_table(dev, ops, sizes, reps, warmup):
    rng = np.random.RandomState(0)
    rows = []
    for k in NETS:
        n = sizes[k]
        p = dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32) * 0.05)
        g = dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32) * 1e-3)
        st = [dev.zeros((1, n, 1, 1)) for _ in range(3)]
        hyper = dev.tensor(np.array([1e-5, 0.0], np.float32))
        for rule in RULES:
            run = launcher(ops, rule, p, g, st[:RULES[rule][0]], n, hyper)
            for _ in range(warmup):
                run()
            for r in range(reps):
                dev.timer_start(r)
                run()
                dev.timer_stop(r)
            ms = float(np.median([dev.timer_ms(r) for r in range(reps)]))
            tbs = bytes_per_param(rule) * n / (ms * 1e-3) / 1e12
            rows.append({'net': k, 'n': n, 'rule': rule, 'bytes_per_param': bytes_per_param(rule), 'ms': ms, 'TB_s': tbs})
            print("%-10s n=%-9d %-18s %2d B/param  %8.4f ms  %5.2f TB/s" % (k, n, rule, bytes_per_param(rule), ms, tbs),
                  flush=True)
        del p, g, st
    return rows


def step_time(rule, steps):
    """ms per joint train step with opt=<rule> (runs in a child process of its own: one model per process)"""
    from bench import synthetic_batch
    from gan_heightmaps_amd import device, updates
    from gan_heightmaps_amd.experiments import make_model
    dev = device.Device(0)
    m = make_model('test1_nobn_bilin_both', device=dev, use_graph='recorded', seed=0, verbose=False, dtype='bf16x3',
                   opt=getattr(updates, rule), opt_args={'learning_rate': updates.shared(np.float32(1e-4))})
    eng = m.engine
    b = eng.built(4)
    eng._upload(b, *synthetic_batch(4, 1000, 512, seed=1000))
    for _ in range(5):                      # eager, record, warm replays
        eng.enqueue_train(b)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.enqueue_train(b)
    eng.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def step_ab(steps, blocks=3):
    """opt=rmsprop and opt=amsgrad alternately, each block in a fresh child process"""
    import subprocess
    ms = {'rmsprop': [], 'amsgrad': []}
    for _ in range(blocks):
        for rule in ms:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", rule, "--step-ab", str(steps)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit("step timing of opt=%s failed (rc %d):\n%s" % (rule, out.returncode, out.stderr[-2000:]))
            ms[rule].append(float(out.stdout.strip().splitlines()[-1]))
    res = {r: {'ms_per_step_blocks': v, 'ms_per_step': float(np.median(v))} for r, v in ms.items()}
    res['steps_per_block'] = steps
    res['amsgrad_minus_rmsprop_ms'] = res['amsgrad']['ms_per_step'] - res['rmsprop']['ms_per_step']
    res['relative'] = res['amsgrad_minus_rmsprop_ms'] / res['rmsprop']['ms_per_step']
    for r in ms:
        print("step opt=%-8s %.3f ms (blocks %s)" % (r, res[r]['ms_per_step'], ", ".join("%.3f" % v for v in ms[r])), flush=True)
    print("amsgrad - rmsprop: %+.3f ms (%+.2f %%)" % (res['amsgrad_minus_rmsprop_ms'], 100 * res['relative']), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-ab", type=int, default=0, metavar="STEPS")
    ap.add_argument("--out", default=None, help="write the results as JSON")
    ap.add_argument("--step-only", default=None, help=argparse.SUPPRESS)      # (child process of --step-ab)
    args = ap.parse_args(argv)
    if args.step_only:
        print(step_time(args.step_only, args.step_ab))
        return 0
    # the step A/B first: its child processes start before this one opens the device
    ab = step_ab(args.step_ab) if args.step_ab else None
    from gan_heightmaps_amd import device
    from gan_heightmaps_amd.experiments import make_model
    if device.device_count() == 0:
        sys.exit("opt_update_bench.py: no HIP device visible")
    dev = device.Device(0)
    # the buffer sizes of the product's parameter stores (the trained part of each net's flat buffer)
    m = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False)
    sizes = {k: m.engine.stores[k].n_train for k in NETS}
    del m
    res = {'device': dev.info(), 'reps': args.reps, 'warmup': args.warmup, 'sizes': sizes,
           'kernels': kernel_table(dev, device.Ops(dev), sizes, args.reps, args.warmup)}
    if ab:
        res['step_ab'] = ab
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
