#!/usr/bin/env python
"""Wall time and size of one training-state checkpoint of experiment test1_nobn_bilin_both with opt=adam (MI355X).

    python tools/checkpoint_bench.py [--levels 0,1,9] [--dir DIR] [--out FILE]

Builds the full-size model with Adam, takes two train steps on a synthetic batch (so that the moments are not the zeros
of a fresh run, which compress to nothing), then per gzip level: Pix2Pix.save_checkpoint and load_checkpoint into the
same model, each timed on the wall clock, and the file size.  Prints one JSON object (and writes it to ``--out``).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="0,1,9", help="gzip levels to time, comma-separated")
    ap.add_argument("--dir", default=None, help="where the checkpoint files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gan_heightmaps_amd import experiments, updates
    from gan_heightmaps_amd.init import floatX
    from oracle import step as ostep
    m = experiments.make_model('test1_nobn_bilin_both', opt=updates.adam,
                               opt_args={'learning_rate': updates.shared(floatX(1e-4))}, verbose=False, seed=1)
    cfg = ostep.default_cfg()
    for i in range(2):
        m.train_fn(*ostep.synthetic_batch(4, cfg, seed=i))
    eng = m.engine
    n_train = sum(eng.stores[k].n_train for k in eng.stores if k in eng.hyper)
    out = {'experiment': 'test1_nobn_bilin_both', 'opt': 'adam', 'n_train': int(n_train),
           'fp32_state_bytes': int(4 * n_train * (1 + len(eng.opt_rule.slots))), 'levels': {}}
    d = args.dir or tempfile.mkdtemp()
    for lvl in [int(x) for x in args.levels.split(",")]:
        m.checkpoint_compresslevel = lvl
        path = os.path.join(d, "bench_%d.model" % lvl)
        t0 = time.perf_counter()
        m.save_checkpoint(path, epoch=1)
        t1 = time.perf_counter()
        m.load_checkpoint(path)
        t2 = time.perf_counter()
        out['levels'][lvl] = {'save_s': round(t1 - t0, 2), 'load_s': round(t2 - t1, 2),
                              'file_bytes': os.path.getsize(path)}
        os.remove(path)
        print(json.dumps({lvl: out['levels'][lvl]}), flush=True)
    if not args.dir:
        os.rmdir(d)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
