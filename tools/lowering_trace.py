#!/usr/bin/env python
"""Call trace of the lowering (engine.NetPlan's emitters, step.GanStep's programs) on the host-only policy device: every
program entry and every Ops call it makes, with its arguments, as one digest per case.  Fake addresses come from an
allocation counter, so the digests also pin the order and size of every device allocation the emitters make.  The way to
check that a change of the lowering changes nothing: trace both trees with THIS file and compare the two outputs.

    python tools/lowering_trace.py > after.json
    python tools/lowering_trace.py --root /path/to/a/worktree/of/the/parent > before.json
    python tools/lowering_trace.py --dump corpus/unet_skip/bf16x3          # the canonical trace of one case, to diff

Cases: every graph of tests/lowering_corpus.py in every arithmetic mode (forward, backward with the image-input gradients,
deterministic forward); GanStep.built(4) (the loss programs, both stage programs, the exchange and the updates) for every
arithmetic mode x train mode x one / two streams, on 128-pixel nets and on the 512-pixel headline model; the headline
model's deterministic U-Net inference plan; the headline model in bf16x3 under each environment switch the emitters read;
the data-parallel step of the 128-pixel nets behind a fake communicator (every exchange mode, embedded and captured-graph
form, both ranks of a world of two); and three steps of the asynchronous input pipeline (host batches, resident batches).
Event records and waits, asynchronous uploads and device-to-device copies are traced with the entry that made them."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ENV_SWITCHES = ("GHM_BN_FP32", "GHM_POOL_READ_Y", "GHM_DACT_FP32")
TRAIN_MODES = ("both", "dcgan", "p2p")
EXCHANGE_MODES = ("allreduce", "allreduce_bf16", "rs_ag")


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


def trace_device():
    """tests.fake_device.PolicyDevice whose contexts and events are named by creation counters (the fake device names them by
    id()), logging to the same FakeDevice.pipe_log: an event is 'ev<creating context>.<its counter there>'"""
    from tests.fake_device import FakeDevice, PolicyDevice

    class TraceDevice(PolicyDevice):
        made = 0

        def __init__(self, index=0):
            PolicyDevice.__init__(self, index)
            self.serial = TraceDevice.made
            TraceDevice.made += 1

        def name(self):
            return "ctx%d" % self.serial

        def event_create(self):
            return ("ev", self.serial, PolicyDevice.event_create(self)[2])

        def event_record(self, ev):
            FakeDevice.pipe_log.append(("record", "ev%d.%d" % ev[1:], self.name()))

        def event_wait(self, ev):
            FakeDevice.pipe_log.append(("wait", "ev%d.%d" % ev[1:], self.name()))

        @staticmethod
        def event_sync(ev):
            FakeDevice.pipe_log.append(("host_sync", "ev%d.%d" % ev[1:]))

        def wait_for(self, other):
            FakeDevice.pipe_log.append(("wait_for", other.name(), self.name()))
    return TraceDevice


class _Mark:
    """what the Ops objects and the fake device's pipe_log have gained since the mark was made"""

    def __init__(self, ops_list):
        from tests.fake_device import FakeDevice
        self.ops_list, self.log = ops_list, FakeDevice.pipe_log
        self.before, self.at = [len(o.calls) for o in ops_list], len(self.log)

    def calls(self):
        out = []
        for i, o in enumerate(self.ops_list):
            out += [[i, c[0], render(c[1]), render(c[2])] for c in o.calls[self.before[i]:]]
        return out

    def pipe(self):
        """(a run of waits for ONE event by several contexts is sorted: enqueue_train_uploaded walks a set of contexts, and
        streams that wait for the same event do so in no order)"""
        out = []
        for line in self.log[self.at:]:
            i = len(out)
            while line[0] == "wait" and i and out[i - 1][:2] == ["wait", line[1]] and out[i - 1][2] > line[2]:
                i -= 1
            out.insert(i, render(line))
        return out


def trace_programs(programs, ops_list, devs=()):
    """``programs``: [(name, entries)], all emitted already.  Runs every entry and returns the canonical trace: per entry
    its program, label, arity, meta, side-stream device (index into ``devs``), the Ops calls it made as
    (index into ``ops_list``, method, args, kwargs) and the lines it appended to the fake device's pipe_log."""
    out = []
    for pname, prog in programs:
        for e in prog:
            mark = _Mark(ops_list)
            e[1]()
            dev = None
            if len(e) > 3 and e[3] is not None:
                dev = [k for k, d in enumerate(devs) if d is e[3]][0]
            out.append({"prog": pname, "label": e[0], "arity": len(e), "meta": render(e[2]) if len(e) > 2 else None,
                        "dev": dev, "calls": mark.calls(), "pipe": mark.pipe()})
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
        lines += ["    pipe %s" % json.dumps(line) for line in r.get("pipe", ())]
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
    """the Ops objects and contexts of an engine, the communicator's last"""
    ops = _unique(list(eng.ops) + [sd[1] for sd in eng.side if sd is not None] + [eng.cops])
    devs = _unique(list(eng.devs) + [sd[0] for sd in eng.side if sd is not None] + [eng.cdev])
    return ops, devs


class FakeComm:
    """what GanStep reads of a communicator when it builds a step: its context, the world size and this rank"""

    def __init__(self, dev, world, rank):
        self.dev, self.world, self.rank = dev, world, rank


def _engine_128(dtype, train_mode, two_streams, opt='rmsprop', comm=None, **kw):
    from gan_heightmaps_amd import updates
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.nonlinearities import linear, tanh
    from gan_heightmaps_amd.step import GanStep
    G = dcgan.default_generator(24, True, nch=64, div=[1, 2, 2, 2], initial_size=8)     # 8 -> 128
    Dn = dcgan.default_discriminator(128, True, nch=64, div=[2, 1, 1], nonlinearity=linear)
    U = p2p.g_unet(128, True, False, nf=32, act=tanh, bilinear_upsample=True)
    P = p2p.discriminator(128, True, False, nf=32, act=linear, mul_factor=[1, 2])
    spec = getattr(updates, opt)(learning_rate=updates.shared(1e-4))
    kw.setdefault('use_graph', False)
    mk = trace_device()
    dev = mk()
    if comm is not None:
        kw['comm'] = FakeComm(mk(), *comm)
    return GanStep(dev, G, Dn, U, P, 100, True, 'l1', spec, train_mode, two_streams=two_streams, dtype=dtype, **kw)


def _engine_dp(mode, use_graph, rank, dtype='bf16x3'):
    """the 128-pixel nets as rank ``rank`` of a world of two: a communication context of its own, sub-buckets of 0.25 MB
    (several per net), the gradient streams in the eager form (captured graphs do not fork them); Adam in the sharded form
    (tick entries, two state slots)"""
    return _engine_128(dtype, 'both', True, opt='adam' if mode == 'rs_ag' else 'rmsprop', comm=(2, rank),
                       use_graph=use_graph, side_streams=use_graph is not True, bucket_mb=0.25, exchange_mode=mode)


def _engine_512(dtype, **kw):
    from gan_heightmaps_amd.experiments import make_model
    return make_model('test1_nobn_bilin_both', device=trace_device()(), use_graph=False, seed=0, verbose=False,
                      dtype=dtype, **kw).engine


def trace_step(eng):
    """built(4): both lanes of the loss program and of the train program, the exchange, then both update lists; the
    collective order goes in front, as an entry that calls nothing"""
    b = eng.built(4)
    ops, devs = _engine_lists(eng)
    order = [("xchg_order", lambda: None, [list(t) for t in b.xchg_order])]
    return trace_programs([("plan", order), ("loss0", b.loss_prog[0]), ("loss1", b.loss_prog[1]),
                           ("train0", b.train_compute[0]), ("train1", b.train_compute[1]), ("exchange", b.exchange),
                           ("update0", b.update[0]), ("update1", b.update[1])], ops, devs)


def _trace_calls(eng, steps):
    """``steps``: [(label, function)], host calls on an engine (each may issue whole programs): one trace record per call,
    with every Ops call and pipe_log line it made"""
    ops, devs = _engine_lists(eng)
    out = []
    for label, fn in steps:
        mark = _Mark(ops)
        fn()
        out.append({"prog": "pipeline", "label": label, "arity": 2, "meta": None, "dev": None, "calls": mark.calls(),
                    "pipe": mark.pipe()})
    return out


def trace_pipelined(eng, steps=3):
    """train_pipelined over ``steps`` host batches (batch i filled with i): per step the enqueue, the upload of the next batch
    and the read of the losses; then close_pipeline"""
    batches = [(np.full((4, 24), i, np.float32), np.full((4, 1, 128, 128), i, np.float32), np.full((4, 3, 128, 128), i, np.float32))
               for i in range(steps)]
    it = eng.train_pipelined(iter(batches))
    calls = [("step%d" % i, lambda: next(it)) for i in range(steps)]
    return _trace_calls(eng, calls + [("end", lambda: next(it, None)), ("close", eng.close_pipeline)])


def trace_resident(eng, steps=3):
    """bench.py's timed loop: resident batches copied into alternating plans (slots 0 / 1) on the copy stream, each step run by
    enqueue_train_uploaded"""
    plans = [eng.built(4, 0), eng.built(4, 1)]
    dev = eng.devs[0]
    pool = [(dev.empty((4, 24)), dev.empty((4, 1, 128, 128)), dev.empty((4, 3, 128, 128))) for _ in range(3)]
    calls = [("upload0", lambda: eng.upload_resident_async(plans[0], *pool[0]))]
    for k in range(steps):
        calls.append(("step%d" % k, lambda k=k: eng.enqueue_train_uploaded(plans[k & 1])))
        calls.append(("upload%d" % (k + 1), lambda k=k: eng.upload_resident_async(plans[(k + 1) & 1], *pool[(k + 1) % 3])))
    return _trace_calls(eng, calls + [("close", eng.close_pipeline)])


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
    for mode in EXCHANGE_MODES:
        for ug in (False, True):
            for rank in (0, 1):
                out["dp128/%s/%s/rank%d" % (mode, "graph" if ug else "embedded", rank)] = \
                    lambda mode=mode, ug=ug, rank=rank: trace_step(_engine_dp(mode, ug, rank))
    out["dp128/allreduce_f16/embedded/rank1"] = lambda: trace_step(_engine_dp('allreduce', False, 1, dtype='f16'))
    out["pipeline128/host_batches"] = lambda: trace_pipelined(_engine_128('bf16x3', 'both', True))
    out["pipeline128/resident"] = lambda: trace_resident(_engine_128('bf16x3', 'both', True))
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
