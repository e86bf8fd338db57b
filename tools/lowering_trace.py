#!/usr/bin/env python
"""Call trace of the lowering (engine.NetPlan's emitters, step.GanStep's programs) on the host-only policy device: every
program entry and every Ops call it makes, with its arguments, as one digest per case.  Fake addresses come from an
allocation counter, so the digests also pin the order and size of every device allocation the emitters make.  The way to
check that a change of the lowering changes nothing: trace both trees with THIS file and compare the two outputs.

    python tools/lowering_trace.py > after.json
    python tools/lowering_trace.py --root /path/to/a/worktree/of/the/parent > before.json
    python tools/lowering_trace.py --dump corpus/unet_skip/bf16x3          # the canonical trace of one case, to diff

Cases: every graph of tests/lowering_corpus.py in every arithmetic mode (forward, backward with the image-input gradients,
deterministic forward); GanStep.built(4) (both stage programs and the updates) for every arithmetic mode x train mode x
one / two streams, on 128-pixel nets and on the 512-pixel headline model; the headline model's deterministic U-Net
inference plan; and the headline model in bf16x3 under each environment switch the emitters read."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ENV_SWITCHES = ("GHM_BN_FP32", "GHM_POOL_READ_Y", "GHM_DACT_FP32")
TRAIN_MODES = ("both", "dcgan", "p2p")


def use_root(root=None):
    """import the package and tests/ from checkout ``root`` (default: the one this file lives in)"""
    root = os.path.abspath(root or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    return root


def render(v):
    """a value of an entry or an Ops call as JSON-able data; a value of a type not listed here is an error (nothing may be
    compared as 'some object')"""
    from gan_heightmaps_amd.device import DevTensor, QTensor
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, DevTensor):
        return ["DevTensor", v.ptr, list(v.shape), v.nstride]
    if isinstance(v, QTensor):
        return ["QTensor", v.ptr, list(v.shape), v.dtype, v.nstride, v.pstride]
    if isinstance(v, ctypes.Structure):
        return [type(v).__name__, {f[0]: render(getattr(v, f[0])) for f in v._fields_}]
    if isinstance(v, np.ndarray):
        return ["ndarray", list(v.shape), str(v.dtype), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()]
    if isinstance(v, (tuple, list)):
        return [render(x) for x in v]
    if isinstance(v, dict):
        return {(k if isinstance(k, str) else json.dumps(render(k))): render(x) for k, x in v.items()}
    raise TypeError("lowering trace: value of unknown type %s" % type(v).__name__)


def trace_programs(programs, ops_list, devs=()):
    """``programs``: [(name, entries)], all emitted already.  Runs every entry and returns the canonical trace: per entry
    its program, label, arity, meta, side-stream device (index into ``devs``) and the Ops calls it made as
    (index into ``ops_list``, method, args, kwargs)."""
    out = []
    for pname, prog in programs:
        for e in prog:
            before = [len(o.calls) for o in ops_list]
            e[1]()
            calls = []
            for i, o in enumerate(ops_list):
                calls += [[i, c[0], render(c[1]), render(c[2])] for c in o.calls[before[i]:]]
            dev = None
            if len(e) > 3 and e[3] is not None:
                dev = [k for k, d in enumerate(devs) if d is e[3]][0]
            out.append({"prog": pname, "label": e[0], "arity": len(e), "meta": render(e[2]) if len(e) > 2 else None,
                        "dev": dev, "calls": calls})
    return out


def text(trace):
    """the canonical trace as text, one entry or call per line"""
    if isinstance(trace, str):
        return "refused: %s\n" % trace
    lines = []
    for r in trace:
        lines.append("%s %s arity=%d dev=%s meta=%s" % (r["prog"], r["label"], r["arity"], r["dev"],
                                                        json.dumps(r["meta"], sort_keys=True)))
        lines += ["    ops[%d].%s args=%s kw=%s" % (c[0], c[1], json.dumps(c[2], sort_keys=True),
                                                    json.dumps(c[3], sort_keys=True)) for c in r["calls"]]
    return "\n".join(lines) + "\n"


def digest(trace):
    return hashlib.sha256(text(trace).encode()).hexdigest()


# ---- the cases ---------------------------------------------------------------------------------------------------------
def trace_corpus(name, dtype):
    """one graph of the corpus in one mode, as tests/test_lowering_corpus.py lowers it; a refusal is its message"""
    from tests import lowering_corpus as LC
    from tests.test_lowering_corpus import CorpusDevice, CorpusOps
    g = LC.graph(name)
    dev = CorpusDevice()
    ops = CorpusOps(dev)
    try:
        plan, store, fwd, bwd, gin, seed = LC.plan_graph(dev, ops, g, dtype)
        det = []
        plan.emit_forward(det, deterministic=True)
    except NotImplementedError as e:
        return str(e)
    return trace_programs([("fwd", fwd), ("bwd", bwd), ("det", det)], [ops], [dev])


def _unique(items):
    out = []
    for i in items:
        if i is not None and not any(i is o for o in out):
            out.append(i)
    return out


def _engine_lists(eng):
    ops = _unique(list(eng.ops) + [sd[1] for sd in eng.side if sd is not None])
    devs = _unique(list(eng.devs) + [sd[0] for sd in eng.side if sd is not None])
    return ops, devs


def _engine_128(dtype, train_mode, two_streams):
    from gan_heightmaps_amd import updates
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.nonlinearities import linear, tanh
    from gan_heightmaps_amd.step import GanStep
    from tests.fake_device import PolicyDevice
    G = dcgan.default_generator(24, True, nch=64, div=[1, 2, 2, 2], initial_size=8)     # 8 -> 128
    Dn = dcgan.default_discriminator(128, True, nch=64, div=[2, 1, 1], nonlinearity=linear)
    U = p2p.g_unet(128, True, False, nf=32, act=tanh, bilinear_upsample=True)
    P = p2p.discriminator(128, True, False, nf=32, act=linear, mul_factor=[1, 2])
    spec = updates.rmsprop(learning_rate=updates.shared(1e-4))
    return GanStep(PolicyDevice(), G, Dn, U, P, 100, True, 'l1', spec, train_mode, use_graph=False,
                   two_streams=two_streams, dtype=dtype)


def _engine_512(dtype, **kw):
    from gan_heightmaps_amd.experiments import make_model
    from tests.fake_device import PolicyDevice
    return make_model('test1_nobn_bilin_both', device=PolicyDevice(), use_graph=False, seed=0, verbose=False,
                      dtype=dtype, **kw).engine


def trace_step(eng):
    """built(4): both lanes of the train program, then both update lists"""
    b = eng.built(4)
    ops, devs = _engine_lists(eng)
    return trace_programs([("train0", b.train_compute[0]), ("train1", b.train_compute[1]),
                           ("update0", b.update[0]), ("update1", b.update[1])], ops, devs)


def trace_infer(eng):
    """the deterministic U-Net forward plan (what gen_fn_det and the tiled texturing run)"""
    plan, prog = eng._infer_plan('p2p_gen', 4, True)
    ops, devs = _engine_lists(eng)
    return trace_programs([("infer", prog)], ops, devs)


def _with_env(var, fn):
    def run():
        assert var not in os.environ, var
        os.environ[var] = "1"
        try:
            return fn()
        finally:
            os.environ.pop(var)
    return run


def cases():
    """-> {case name: function returning its canonical trace}, in a fixed order"""
    from tests import lowering_corpus as LC
    out = {}
    for name in LC.NAMES:
        for m in LC.MODES:
            out["corpus/%s/%s" % (name, m)] = lambda name=name, m=m: trace_corpus(name, m)
    for size, make in (("step128", _engine_128), ("step512", lambda dt, tm, ts: _engine_512(dt, train_mode=tm, two_streams=ts))):
        for m in LC.MODES:
            for tm in TRAIN_MODES:
                for ts in (False, True):
                    out["%s/%s/%s/%s" % (size, m, tm, "two_streams" if ts else "one_stream")] = \
                        lambda make=make, m=m, tm=tm, ts=ts: trace_step(make(m, tm, ts))
    for m in LC.MODES:
        out["infer512/%s" % m] = lambda m=m: trace_infer(_engine_512(m))
    for var in ENV_SWITCHES:
        out["env512/%s" % var] = _with_env(var, lambda: trace_step(_engine_512('bf16x3')))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", help="checkout to import the package and tests/ from (default: this file's)")
    ap.add_argument("--dump", metavar="CASE", help="print the canonical trace of one case instead of the digests")
    ap.add_argument("--only", metavar="PREFIX", help="only the cases whose name starts with PREFIX")
    args = ap.parse_args()
    for var in ENV_SWITCHES:
        if var in os.environ:
            sys.exit("unset %s first: the tool sets it itself, for one case" % var)
    use_root(args.root)
    todo = cases()
    if args.dump:
        sys.stdout.write(text(todo[args.dump]()))
        return
    digests, resumed = {}, args.only is not None
    for name, fn in todo.items():
        if args.only and not name.startswith(args.only):
            continue
        tr = fn()
        digests[name] = digest(tr)
        if name.startswith("step") and any(r["label"] == "per_sample_ratio" for r in tr):
            resumed = True
    # the resume= path of emit_backward is taken whenever a discriminator returns one scalar per sample: keep it traced
    assert resumed, "no GanStep case emitted a per_sample_ratio entry: emit_backward(resume=) is no longer traced"
    json.dump(digests, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
