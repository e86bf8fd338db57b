"""The two-stage GAN step of the reference (/root/reference/pix2pix.py:87-147) as static device programs.

One ``GanStep`` owns the four networks' parameters in HBM and, per batch size, a set of NetPlans wired the
way ``Pix2Pix.__init__`` wires the Theano graph:
  * G(z) is evaluated once and written straight into the second half of the DCGAN discriminator's input
    batch, so D(X) and D(G(z)) run as ONE 2B-sample pass (D has no BatchNorm in any reference experiment),
  * U(X) is written straight into channels 1.. of the second half of the PatchGAN's concat buffer,
  * four gradient roots, each w.r.t. its own net's parameters, all at the pre-update parameters:
    D-loss backward on the 2B batch (weights + data gradients), G-loss backward through D on the fake half
    only (data gradients only), then through G; same for PatchGAN / U-Net with alpha * L1 added,
  * per net: (data-parallel: one RCCL all-reduce of the flat gradient buffer) then one optimiser kernel.

The DCGAN stage and the pix2pix stage of a step share nothing but the read-only input X (pix2pix.py:99: the
U-Net consumes real X, not G(z)), so they are enqueued on TWO HIP streams (two ghm contexts on the same
device): the low-parallelism layers of one stage (4x4 .. 16x16 maps, reductions) overlap the other stage's
big convolutions.
"""
import os

import numpy as np

from . import layers as L
from .device import Ops
from .engine import NetPlan, ParamStore
from .input_pipeline import InputPipeline
from .step_build import EMA_NETS, LANE_OF, StepBuilder

TRAIN_KEYS = ['dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_recon', 'p2p_disc']


class OptRule:
    """one lasagne.updates rule as the engine runs it: the names of its per-parameter fp32 state buffers, whether it
    advances the step counter hyper[1] (ghm_adam_tick, behind the update), and its launch
    ``run(ops, p, g, states, n, hyper, hp, grad_scale)`` with ``states`` in ``slots`` order"""

    def __init__(self, slots, ticks, run):
        self.slots, self.ticks, self.run = slots, ticks, run


def _opt_update(kind, consts):
    return lambda o, p, g, s, n, hy, hp, gs: o.opt_update(kind, p, g, s, n, hy, [hp[c] for c in consts], gs)


# keyed by OptimizerSpec.kind; update entries are labelled <kind>_<net> / <kind>_shard_<bucket>, ticks <kind>_tick_<net>
OPT_RULES = {
    'rmsprop': OptRule(('acc',), False,
                       lambda o, p, g, s, n, hy, hp, gs: o.rmsprop(p, g, s[0], n, hy, hp['rho'], hp['epsilon'], gs)),
    'adam': OptRule(('m', 'v'), True,
                    lambda o, p, g, s, n, hy, hp, gs: o.adam(p, g, s[0], s[1], n, hy, hp['beta1'], hp['beta2'],
                                                             hp['epsilon'], gs)),
    'sgd': OptRule((), False, _opt_update('sgd', ())),
    'momentum': OptRule(('velocity',), False, _opt_update('momentum', ('momentum',))),
    'nesterov_momentum': OptRule(('velocity',), False, _opt_update('nesterov_momentum', ('momentum',))),
    'adagrad': OptRule(('accu',), False, _opt_update('adagrad', ('epsilon',))),
    'adadelta': OptRule(('accu', 'delta_accu'), False, _opt_update('adadelta', ('rho', 'epsilon'))),
    'adamax': OptRule(('m', 'u'), True, _opt_update('adamax', ('beta1', 'beta2', 'epsilon'))),
    'amsgrad': OptRule(('m', 'v', 'vhat'), True, _opt_update('amsgrad', ('beta1', 'beta2', 'epsilon'))),
}


def opt_rule(kind):
    if kind not in OPT_RULES:
        raise ValueError("unknown optimiser kind %r (known: %s)" % (kind, ", ".join(OPT_RULES)))
    return OPT_RULES[kind]


def crc_range(comm, crc):
    """(min, max) over the ranks of a 32-bit CRC (every rank calls it; ``comm`` None: this process alone)"""
    if comm is None:
        return crc, crc
    lo16, hi16 = float(crc & 0xffff), float(crc >> 16)          # exactly representable in fp32
    mx = (comm.max_scalar(hi16), comm.max_scalar(lo16))
    mn = (-comm.max_scalar(-hi16), -comm.max_scalar(-lo16))
    return (int(mn[0]) << 16 | int(mn[1])), (int(mx[0]) << 16 | int(mx[1]))


STATE_NETS = ('dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc')


def _interleave(a, b):
    """merge two launch lists so that both streams are fed from the start (proportional round-robin)"""
    out, i, j = [], 0, 0
    while i < len(a) or j < len(b):
        if j >= len(b) or (i < len(a) and i * len(b) <= j * len(a)):
            out.append((0, a[i]))
            i += 1
        else:
            out.append((1, b[j]))
            j += 1
    return out


class _EmaWeights:
    """the context manager GanStep.ema_weights() returns"""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        eng = self.eng
        eng._live_only("ema_weights")       # (nested entry)
        eng._swap_ema()
        eng._in_ema = True
        return eng

    def __exit__(self, *exc):
        self.eng._in_ema = False
        self.eng._swap_ema()
        return False


class GanStep:
    def __init__(self, dev, dcgan_gen, dcgan_disc, p2p_gen, p2p_disc, alpha, lsgan, reconstruction, opt_spec,
                 train_mode='both', comm=None, use_graph=True, two_streams=True, force_exchange=False,
                 side_streams=None, dtype='bf16x3', bucket_mb=None, exchange_mode=None, ema=None):
        self.dev = dev
        # exponential moving average of the two generators' parameters, kept on the device behind every update (DESIGN
        # §4o): the decay in [0, 1), or None = no average, nothing allocated, the step's program as it always was
        if ema is not None and not (0.0 <= float(np.float32(ema)) < 1.0):
            raise ValueError("ema must be a decay in [0, 1) or None, not %r" % (ema,))
        self.ema = None if ema is None else float(ema)         # (the kernel takes it rounded to fp32)
        self._in_ema = False                # inside ema_weights(): w and ema are exchanged
        # form of the data-parallel exchange: 'allreduce' (every rank sums every gradient and runs the whole
        # optimiser), 'allreduce_bf16' (the same program with every gradient sub-bucket rounded to bf16 for the trip: half the
        # bytes on the xGMI links, a REDUCED-PRECISION exchange, opt-in; for the first multi-GPU node to A/B) or 'rs_ag'
        # (sharded update: a sub-bucket is reduce-SCATTERED, each rank runs RMSprop / Adam on its 1 / world
        # slice of parameters + state, and the updated slices are all-gathered -- the same bytes on the links, 1 / world of
        # the optimiser's 1.13 GB / step per rank)
        self.exchange_mode = exchange_mode or os.environ.get('GHM_EXCHANGE', 'allreduce')
        assert self.exchange_mode in ('allreduce', 'allreduce_bf16', 'rs_ag'), self.exchange_mode
        # data-parallel exchange: a net's gradient bucket travels as sub-buckets of at least this many bytes, each
        # all-reduced as soon as the backward pass has completed it (step_build.py: cut_buckets, BucketSender)
        self.bucket_bytes = int(float(bucket_mb if bucket_mb is not None else os.environ.get('GHM_BUCKET_MB', 32)) * 2 ** 20)
        # arithmetic of the convolution products (include/ghm.h GHM_DTYPE_*): 'bf16x3' (default) = the reference's floatX by
        # operand splitting (three exact bf16 pieces per operand, csrc/conv_split.hip: fp32-accurate); 'f32' = the same on the
        # fp32 matrix instruction; 'bf16' / 'f16' = BASELINE configs 4 / 5 (matrix-core operands rounded, fp32 accumulation,
        # fp32 tensors and optimiser)
        self.dtype = dtype
        # fp16 operands underflow below 6e-8 and the per-pixel gradients of the 512x512 layers sit around 1e-6..1e-9:
        # the loss-gradient seeds are scaled (initially by 2^15) and the optimiser divides the scale out again (every
        # gradient kernel is linear in its seed; gradients in HBM are fp32, so the scale costs nothing).  The DCGAN
        # discriminator's output is linear and unbounded, so a fixed scale can push a gradient operand beyond the fp16
        # range (65504 -> inf -> nan in the fp32 sums): the scale is DYNAMIC, per stage (the two stages are independent
        # loss graphs) and entirely device state -- ghm_grad_check flags a non-finite gradient bucket, the optimiser
        # kernels skip the update of a flagged step, ghm_loss_scale_update halves / regrows the scale (include/ghm.h) --
        # so a recorded / captured step adapts without a host round trip.  bf16 has fp32's range: no scale.
        self.init_loss_scale = 32768.0 if dtype == 'f16' else 1.0
        self.ls_growth_interval, self.ls_min, self.ls_max = 2000, 1.0, 2.0 ** 24
        self._ls_state = []                 # [(Device, DevTensor of 8 floats)] one per stage stream
        # how a step is issued: False = eager (one C call per kernel), True = one captured HIP graph per stage stream,
        # 'recorded' = the eager multi-stream launch sequence recorded once in the library and replayed by ONE
        # ghm_step_run call per step (side streams, communication stream and collectives included)
        assert use_graph in (True, False, 'recorded')
        if side_streams is None:            # forked branches replay slowly inside a HIP graph: not in graph mode
            side_streams = (use_graph is not True) and two_streams
        if side_streams and use_graph is True:
            raise ValueError("side_streams needs use_graph=False or 'recorded'")
        self._open_streams(dev, two_streams, side_streams, dtype)
        self.nets = {'dcgan_gen': dcgan_gen, 'dcgan_disc': dcgan_disc, 'p2p_gen': p2p_gen,
                     'p2p_disc': p2p_disc["out"]}
        self.p2p_disc_inputs = p2p_disc["inputs"]
        self.alpha, self.lsgan, self.reconstruction = float(alpha), bool(lsgan), reconstruction
        self.opt_spec, self.train_mode = opt_spec, train_mode
        self.use_graph = use_graph
        self._attach_comm(comm, force_exchange)
        self.stores = {k: ParamStore(self.devs[LANE_OF[k]], L.get_all_params(v), pad_to=self.shard_unit)
                       for k, v in self.nets.items()}
        # per-net optimiser state + hyper-parameter scalars [lr, t] in HBM
        self.hyper = {}
        self.opt_rule = opt_rule(opt_spec.kind)
        lr = float(opt_spec.learning_rate.get_value()) if hasattr(opt_spec.learning_rate, 'get_value') \
            else float(opt_spec.learning_rate)
        for k, st in self.stores.items():
            d = self.devs[LANE_OF[k]]
            self.hyper[k] = d.tensor(np.array([lr, 0.0], np.float32))
            st.opt_state = {name: d.zeros((1, st.n_pad, 1, 1)) for name in self.opt_rule.slots}
        if hasattr(opt_spec.learning_rate, '_listeners'):
            opt_spec.learning_rate._listeners.append(self.set_lr)
        if self.ema is not None:
            for k in EMA_NETS:              # n_pad floats on the net's own lane, zeroed; the average starts at the weights
                self.stores[k].ema = self.devs[LANE_OF[k]].zeros((1, self.stores[k].n_pad, 1, 1))
            self._copy_w_to_ema(EMA_NETS)
        self.losses_dev = dev.zeros((1, 8, 1, 1))
        self._built = {}                    # {B or (B, slot): the plan set} (step_build.py)
        self._infer = {}
        self._subgraph = {}
        self._param_ticks = 0
        self._rng_counters = {}             # {('G' / 'U', B): dropout step counter of the train plans}, shared by both slots
        self._pending_counters = None       # counters of a restored checkpoint whose plans are not built yet
        self.xchg_bf16 = {}                 # {net key: address of its bf16 exchange buffer} (exchange_mode 'allreduce_bf16')
        self._lev = self._gev = None        # events on the communication stream, made at first use (_losses_event, _gather_events)
        self.pipeline = InputPipeline(self)     # opens its copy stream at the first upload

    def _open_streams(self, dev, two_streams, side_streams, dtype):
        mk = type(dev)                      # second / side streams are further contexts of the same kind on this GPU
        mkops = getattr(dev, 'ops_class', Ops)
        self.devs = [dev, mk(dev.index) if two_streams else dev]
        self.ops = [mkops(self.devs[0]), mkops(self.devs[1])]
        if dtype == 'f16':
            for d in ([self.devs[0]] if self.devs[1] is self.devs[0] else self.devs):
                t = d.tensor(np.array([self.init_loss_scale, 1.0 / self.init_loss_scale, 0, 0, 0, 0, 0, 0], np.float32))
                d.set_loss_scale_state(t)
                self._ls_state.append((d, t))
        # optional GRADIENT stream for the weight / bias gradients of both stages (engine.NetPlan side=).  ONE stream for
        # the two stages, not one each: three MFMA-heavy kernels at a time (stage A, stage B, one weight gradient) is what
        # the chip runs best -- with a gradient stream per stage the two weight-gradient kernels share CUs with each other
        # and the step is 3 % slower (162.5 vs 167.6 img/s fp32, 435 vs 465 bf16).  (A per-stage pair used to measure
        # the same as the shared stream only because ROCm's default of four hardware queues happened to put the two
        # gradient streams on one queue; GHM_GRAD_STREAM_PER_STAGE=1 restores the pair for measurements.)
        self.side = [None, None]
        if side_streams:
            per_stage = two_streams and bool(os.environ.get('GHM_GRAD_STREAM_PER_STAGE'))
            sd = [mk(dev.index), mk(dev.index) if per_stage else None]
            if sd[1] is None:
                sd[1] = sd[0]
            self.side = [(sd[0], mkops(sd[0])), (sd[1], mkops(sd[1]))]

    def _attach_comm(self, comm, force_exchange):
        self.comm = comm
        self.world = comm.world if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        # the communicator's context is the COMMUNICATION stream: a Comm made on its own Device of the same GPU lets
        # the bucket all-reduces run beside the rest of the backward pass; a Comm made on ``dev`` itself serialises
        # them on stream A.  Either way it must be this GPU, or every rank would reduce somebody else's buffers.
        self.cdev = comm.dev if comm is not None else None
        self.cops = getattr(self.cdev, 'ops_class', Ops)(self.cdev) if comm is not None else None
        if comm is not None and getattr(comm.dev, 'index', None) != getattr(self.dev, 'index', None):
            raise ValueError("comm was initialised on device %r, the step runs on device %r"
                             % (getattr(comm.dev, 'index', None), getattr(self.dev, 'index', None)))
        # data-parallel code path (stream hand-over, RCCL all-reduce, updates on stream A) even with one rank:
        # lets a single-GPU box exercise exactly what N ranks run
        self.exchange = self.world > 1 or (force_exchange and comm is not None)
        self.sharded = self.exchange and self.exchange_mode == 'rs_ag'
        if self.sharded and self.dtype == 'f16':
            raise NotImplementedError("exchange_mode='rs_ag' with the fp16 dynamic loss scale: every rank would check only its "
                                      "own gradient shard for overflow; use bf16 (no scale) or the all-reduce form")
        if self.sharded and self.ema is not None:
            raise NotImplementedError("exchange_mode='rs_ag' with ema: the sharded update runs on 1 / world of the parameters "
                                      "per rank, so the average would have to become a sharded slot; use the all-reduce form")
        self.shard_unit = 64 * self.world if self.sharded else 1       # elements: world shards of whole 256-byte lines

    @property
    def param_version(self):
        """moves whenever parameters or BatchNorm running statistics may have changed on the device: every train / loss /
        non-deterministic forward call issued, every host write to a parameter and both edges of ema_weights() (world.py
        keys its chunk cache on it)"""
        return self._param_ticks + sum(st.version for st in self.stores.values())

    def loss_scale_state(self):
        """[{scale, clean_steps, skipped_steps}] per stage stream (fp16 mode; [] otherwise).  Synchronises."""
        self.sync()
        out = []
        for _, t in self._ls_state:
            v = t.numpy().ravel()
            out.append({'scale': float(v[0]), 'clean_steps': int(v[2]), 'skipped_steps': int(v[4])})
        return out

    def restore_loss_scale_state(self, states):
        """checkpointed [{scale, clean_steps, skipped_steps}] per stage stream back into the device records"""
        self.sync()
        for (d, t), st in zip(self._ls_state, states):
            v = t.numpy().ravel()
            v[0], v[1], v[2], v[3], v[4] = st['scale'], 1.0 / st['scale'], st.get('clean_steps', 0), 0, st.get('skipped_steps', 0)
            t.set(v)

    def set_loss_scale(self, scale):
        self.sync()
        for d, t in self._ls_state:
            v = t.numpy().ravel()
            v[0], v[1], v[2], v[3] = scale, 1.0 / scale, 0, 0
            t.set(v)

    @property
    def loss_scale(self):
        """the scale the gradient buffers currently carry (stage A's; the stages only differ after an overflow)"""
        if not self._ls_state:
            return 1.0
        self.sync()
        return float(self._ls_state[0][1].numpy().ravel()[0])

    def sync(self):
        self.devs[0].sync()
        if self.devs[1] is not self.devs[0]:
            self.devs[1].sync()
        if self.cdev is not None and self.cdev is not self.devs[0]:
            self.cdev.sync()
        self.pipeline.sync()                # the copy stream of the input pipeline: no upload may outlive a sync()

    def broadcast_parameters(self, root=0):
        """Make every replica start from rank ``root``'s parameters, BatchNorm state and optimiser state (the
        reference never seeds lasagne's RNG -- SURVEY Appendix A.9 -- so unseeded ranks would otherwise train
        different weights with averaged gradients).  A broadcast is an all-reduce whose other contributions are
        zero: exact, and it needs no further collective in the C ABI."""
        if self.comm is None or self.world == 1:
            return
        self._live_only("broadcast_parameters")
        self._param_ticks += 1
        self.sync()
        for k in ('dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc'):
            st = self.stores[k]
            bufs = [(st.w, st.n_train), (st.s, st.n_state)] + [(t, st.n_train) for _, t in sorted(st.opt_state.items())]
            bufs.append((self.hyper[k], 2))
            if self.ema is not None and k in EMA_NETS:
                bufs.append((st.ema, st.n_train))
            for t, n in bufs:
                if n <= 0:
                    continue
                if self.rank != root:
                    self.cdev.memset_zero(t.ptr, 4 * n)
                self.cops.allreduce_sum(t, n)
        self.sync()

    def replica_checksums(self):
        """(min, max) over the ranks of a CRC of every parameter / state buffer: equal on healthy replicas."""
        import zlib
        self.sync()
        crc = 0
        for k in ('dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc'):
            st = self.stores[k]
            for t in (st.w, st.s) + ((st.ema,) if self.ema is not None and k in EMA_NETS else ()):
                crc = zlib.crc32(t.numpy().tobytes(), crc)
        return crc_range(self.comm if self.world > 1 else None, crc)

    # ---- the exponential moving average of the generators ----------------------------------------
    def _live_only(self, what):
        """inside ema_weights() the parameter buffers hold the average: whatever would move parameters or state is refused"""
        if self._in_ema:
            raise RuntimeError("%s inside ema_weights(): the parameter buffers hold the averaged weights until the block ends"
                               % what)

    def _need_ema(self, what):
        if self.ema is None:
            raise ValueError("%s: this model keeps no average (construct it with ema=<decay>)" % what)

    def _copy_w_to_ema(self, keys):
        for k in keys:
            st = self.stores[k]
            if st.n_train:
                st.dev.d2d(st.ema.ptr, st.w.ptr, 4 * st.n_train)

    def reset_ema(self, keys=EMA_NETS):
        """start the average again from the current weights (after a warm-up; load_model does it for the nets it loads)"""
        self._need_ema("reset_ema")
        self._live_only("reset_ema")
        self.close_pipeline()
        self.sync()
        self._copy_w_to_ema([k for k in keys if k in EMA_NETS])
        self.sync()

    def _swap_ema(self):
        self.close_pipeline()
        self.sync()
        for k in EMA_NETS:
            st = self.stores[k]
            self.ops[LANE_OF[k]].swap_f32(st.w, st.ema, st.n_train)
        self._param_ticks += 1          # param_version: TerrainWorld drops its chunk and head caches
        self.sync()

    def ema_weights(self):
        """``with eng.ema_weights(): ...`` -- inside the block the generators' parameter buffers hold the averaged weights
        (exchanged with the average on the device, and exchanged back on exit, also when the body raises), so everything
        that reads parameters -- the deterministic forwards, generate_chain, texture_heightmap, generate_terrain,
        terrain_world, get_all_param_values, save_model -- sees them with no further change; BatchNorm running statistics
        stay the live ones.  Whatever would move parameters or state raises RuntimeError inside."""
        self._need_ema("ema_weights")
        self._live_only("ema_weights")
        return _EmaWeights(self)

    def ema_values(self, key):
        """get_all_param_values of generator ``key`` with the averaged values in place of the trainable ones (read from the
        average's buffer: nothing is exchanged, param_version does not move)"""
        self._need_ema("ema_values")
        self.sync()
        st = self.stores[key]
        src = st.w if self._in_ema else st.ema          # inside ema_weights() the parameter buffer IS the average
        return [st._from_device_layout(p, st._view(src, p).numpy().ravel()) if p.index[0] == 'w' else st.download(p)
                for p in st.params]

    def set_lr(self, lr):
        self.sync()
        for k, h in self.hyper.items():
            cur = h.numpy().ravel()
            cur[0] = lr
            h.set(cur)

    # ---- training state (checkpoint / resume) ------------------------------------------------------------
    # Everything a step reads besides the parameters and the batch: per net the optimiser slots and hyper = [lr, t], the
    # dropout step counters and the fp16 loss-scale records; with GanStep(ema=decay) the decay and the generators' averages.  Restored IN PLACE: recorded programs and captured graphs hold
    # these buffers' pointers.
    def _counters(self):
        """{(name, batch size): DevTensor} of every dropout counter that exists: the train plans' per (net, B) ('G' / 'U'),
        the non-deterministic forward-only plans' per (net key, B)"""
        out = {k: t for k, t in self._rng_counters.items() if t is not None}
        for (key, B, det), (plan, _) in self._infer.items():
            if not det and plan.rng_counter is not None:
                out[(key, B)] = plan.rng_counter
        return out

    def _apply_pending_counters(self):
        """counters restored before their plan existed take their value when it is built"""
        pend = self._pending_counters
        if not pend:
            return
        for key, t in self._counters().items():
            if key in pend:
                t.set(np.asarray([pend.pop(key)], np.uint32).view(np.float32))

    def _state_header(self):
        return {'kind': self.opt_spec.kind, 'hp': {k: float(v) for k, v in self.opt_spec.hp.items()},
                'dtype': self.dtype, 'train_mode': self.train_mode}

    def training_state(self):
        """the engine's training state as host arrays (see restore_training_state).  Drains the input pipeline and every
        stream first.  Sharded update (rs_ag): a rank's optimiser slots are current on its own shards only -- they are
        all-gathered bucket by bucket first (a collective: every rank calls this), so the state is that of the whole net,
        whatever the world size.  Otherwise the state is replicated and this rank's copy is it."""
        self._live_only("training_state")
        self.close_pipeline()
        self.sync()
        if self.sharded and self.opt_rule.slots:
            plans = [b for b in self._built.values() if b.xchg_order]
            if plans:       # (no step yet: the state is still the zeros every rank started from)
                # the buckets are the same in every plan (they depend on the stores and the bucket size only)
                for label, k, blo, n in plans[0].xchg_order:
                    for s in self.opt_rule.slots:
                        self.cops.all_gather(self.stores[k].opt_state[s].channels(blo, blo + n), n // self.world)
                self.sync()
        state = self._state_header()
        state['nets'] = {}
        for k in STATE_NETS:
            st = self.stores[k]
            state['nets'][k] = {
                'n_train': st.n_train, 'n_state': st.n_state,
                'hyper': self.hyper[k].numpy().ravel()[:2].copy(),
                'slots': {s: st.opt_state[s].numpy().ravel()[:st.n_train].copy() for s in self.opt_rule.slots}}
            if self.ema is not None and k in EMA_NETS:
                state['nets'][k]['ema'] = st.ema.numpy().ravel()[:st.n_train].copy()
        if self.ema is not None:
            state['ema'] = self.ema
        counters = {k: int(t.numpy().ravel()[:1].view(np.uint32)[0]) for k, t in self._counters().items()}
        counters.update(self._pending_counters or {})       # restored, plan not built since
        state['rng_counters'] = counters
        state['loss_scale'] = self.loss_scale_state()
        return state

    def check_training_state(self, state):
        """ValueError naming the first field in which ``state`` does not fit this engine"""
        live = self._state_header()
        for f in ('kind', 'hp', 'dtype', 'train_mode'):
            if state.get(f) != live[f]:
                raise ValueError("training state: %s is %r in the checkpoint, %r in this run" % (f, state.get(f), live[f]))
        for k in STATE_NETS:
            st, sv = self.stores[k], state['nets'].get(k, {})
            for f in ('n_train', 'n_state'):
                if sv.get(f) != getattr(st, f):
                    raise ValueError("training state: %s of %s is %r in the checkpoint, %r in this run"
                                     % (f, k, sv.get(f), getattr(st, f)))
            if sorted(sv['slots']) != sorted(self.opt_rule.slots) or \
                    any(np.asarray(v).size != st.n_train for v in sv['slots'].values()):
                raise ValueError("training state: optimiser slots of %s do not fit %s" % (k, self.opt_spec.kind))
        if len(state.get('loss_scale', [])) != len(self._ls_state):
            raise ValueError("training state: %d loss-scale records in the checkpoint, %d in this run"
                             % (len(state.get('loss_scale', [])), len(self._ls_state)))
        ck = state.get('ema')
        if ck is not None and (self.ema is None or float(ck) != self.ema):
            raise ValueError("training state: ema is %r in the checkpoint, %r in this run" % (ck, self.ema))
        if ck is not None:
            for k in EMA_NETS:
                if np.asarray(state['nets'][k].get('ema', ())).size != self.stores[k].n_train:
                    raise ValueError("training state: the ema values of %s do not fit this run" % k)
        elif self.ema is not None:
            import warnings
            warnings.warn("training state: the checkpoint carries no ema; the averages restart from the loaded weights",
                          RuntimeWarning)

    def restore_training_state(self, state):
        """inverse of training_state, into the existing buffers.  Every rank loads whole buffers (in the sharded form each
        then updates its own shards, as before); padding is zeroed; dropout counters of plans not built yet are applied
        when they are built, counters the checkpoint does not know restart at zero.  The generators' averages (ema) are
        written in place too; from a checkpoint without them they restart from the weights already loaded."""
        self._live_only("restore_training_state")
        self.check_training_state(state)
        self.close_pipeline()
        self.sync()
        for k in STATE_NETS:
            st, sv = self.stores[k], state['nets'][k]
            for s in self.opt_rule.slots:
                full = np.zeros(st.n_pad, np.float32)
                full[:st.n_train] = np.asarray(sv['slots'][s], np.float32)
                st.opt_state[s].set(full)
            self.hyper[k].set(np.asarray(sv['hyper'], np.float32))
            if self.ema is not None and k in EMA_NETS:
                full = np.zeros(st.n_pad, np.float32)
                if state.get('ema') is not None:
                    full[:st.n_train] = np.asarray(sv['ema'], np.float32)
                st.ema.set(full)
                if state.get('ema') is None:        # a checkpoint without an average: it restarts from the loaded weights
                    self._copy_w_to_ema([k])
        self._pending_counters = dict(state['rng_counters'])
        for key, t in self._counters().items():
            t.set(np.asarray([self._pending_counters.pop(key, 0)], np.uint32).view(np.float32))
        if self._ls_state:
            self.restore_loss_scale_state(state['loss_scale'])
        self.sync()

    # ---- building -------------------------------------------------------------------------------------
    def _build(self, B, slot=0):
        return StepBuilder(self, B).build()

    @staticmethod
    def _per_sample_scalar_head(plan, in_layer, dtype='bf16x3'):
        """-> the node that reads ``in_layer`` if the generator-loss gradient through this discriminator may be taken from its
        discriminator-loss pass (see _build), else None: one scalar per sample out, no BatchNorm / InstanceNorm node (batch
        statistics couple the samples; the normalisation backward is not sliced), one conv reader of the input.
        GHM_NO_RANK_ONE=1 keeps the two separate passes (the A/B switch of tests/test_gpu_step.py).
        Not in 'f16': the identity is exact, but the shared pass carries the fake half at the DISCRIMINATOR-loss seed, which is
        smaller than the generator-loss seed by d / (1 - d) (LSGAN; p / (1 - p) with BCE) -- 1e-2 .. 1e-5 once the discriminator
        is winning (pix2pix.py:107-108; results.txt of the reference's run: dcgan_disc 0.0119) -- and fp16 gradient operands
        (range 6e-8 .. 65504 behind the 2^15 loss scale) flush per-pixel gradients that small to zero before the per-sample
        factor multiplies them back up.  fp32 / bf16 pieces have fp32's exponent range: there the error stays relative
        (tests/test_gpu_step.py::test_generator_gradient_shortcut_with_a_confident_discriminator)."""
        if os.environ.get('GHM_NO_RANK_ONE') or (dtype == 'f16' and not os.environ.get('GHM_RANK_ONE_F16')):      # (GHM_RANK_ONE_F16=1: measurement only)
            return None
        if int(np.prod(plan.out.shape[1:])) != 1 or any(n.op == 'bn' for n in plan.order):
            return None
        node = plan.node_of_layer[id(in_layer)]
        if len(node.consumers) != 1 or node.consumers[0].op not in ('conv', 'convpool'):
            return None
        return node.consumers[0]

    def built(self, B, slot=0):
        """the plan set of batch size B; slot 1 = a second, independent set (own activations and input buffers, the same
        parameter stores) for the input pipeline's double buffering"""
        key = B if slot == 0 else (B, slot)
        if key not in self._built:
            self._built[key] = self._build(B, slot)
        return self._built[key]

    # ---- running --------------------------------------------------------------------------------------
    def _upload(self, b, Z, X, Y):
        self.sync()                 # the previous step may still be reading the input buffers
        b.z.set(Z)
        b.x.set(X)
        b.y.set(Y)
        self.sync()

    # ---- asynchronous input pipeline (input_pipeline.py): a copy stream and two plans per batch size ----
    def upload_async(self, b, Z, X, Y):
        self.pipeline.upload_async(b, Z, X, Y)

    def upload_resident_async(self, b, zt, xt, yt):
        self.pipeline.upload_resident_async(b, zt, xt, yt)

    def produce_async(self, b, it, Z_sampler):
        self.pipeline.produce_async(b, it, Z_sampler)

    def enqueue_train_uploaded(self, b, wrap=None):
        self.pipeline.enqueue_train_uploaded(b, wrap)

    def train_pipelined(self, batches):
        self._live_only("train_pipelined")
        return self.pipeline.train_pipelined(batches)

    def train_pipelined_from_iterator(self, it, Z_sampler, steps):
        self._live_only("train_pipelined_from_iterator")
        return self.pipeline.train_pipelined_from_iterator(it, Z_sampler, steps)

    def close_pipeline(self):
        self.pipeline.close()

    def _losses_event(self):
        """persistent event on the communication stream: "the loss all-reduce of the last step has read losses_dev" """
        if self._lev is None:
            self._lev = self.cdev.event_create()
        return self._lev

    def _gather_events(self):
        """one persistent event per net on the communication stream: "this net's updated parameters are gathered" """
        if self._gev is None:
            self._gev = {k: self.cdev.event_create() for k in ('dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc')}
        return self._gev

    def _bind_loss_scale(self):
        """(re)attach this engine's dynamic loss-scale state to its contexts, or detach what another engine left there: the
        contexts are the caller's and several engines may live on one (an fp16 engine's state on it would scale a later
        engine's loss seeds by 2^15; found by running a bf16x2 model after an fp16 one on one Device).  The state pointer is
        read when a launch is issued or recorded, so binding at every issue point is enough -- two host calls."""
        mine = {id(d): t for d, t in self._ls_state}
        for d in {id(d): d for d in self.devs}.values():
            if hasattr(d, 'set_loss_scale_state'):
                d.set_loss_scale_state(mine.get(id(d)))

    def _run_lanes(self, b, name, lanes, wrap=None):
        """Run one launch list per stream: eager (interleaved so both streams fill) on the first call,
        captured into one HIP graph per stream on the second, replayed afterwards.  ``wrap(lane, entry)``
        replaces the plain call (used by bench.py to bracket kernels with HIP events; implies eager)."""
        self._bind_loss_scale()
        if wrap is not None or self.use_graph is not True:
            for lane, e in _interleave(lanes[0], lanes[1]):
                if wrap is not None:
                    wrap(lane, e)
                else:
                    e[1]()
            return
        n = b.calls.get(name, 0)
        b.calls[name] = n + 1
        if n == 0:
            for lane, e in _interleave(lanes[0], lanes[1]):
                e[1]()
            return
        if name not in b.graphs:
            gs = []
            for lane in (0, 1):
                if not lanes[lane]:
                    gs.append(None)
                    continue
                self.devs[lane].capture_begin()
                try:
                    for e in lanes[lane]:
                        e[1]()
                finally:
                    gs.append(self.devs[lane].capture_end())
            b.graphs[name] = gs
            stages = [(self.devs[lane], g) for lane, g in enumerate(gs) if g is not None]
            b.steps[name] = type(self.devs[0]).step_build(stages) if stages else None
        if b.steps.get(name) is not None:
            type(self.devs[0]).step_run(b.steps[name])          # the whole stage-parallel step: one C call

    def _read_losses(self):
        self.sync()
        v = self.losses_dev.numpy().ravel()[:5].astype(np.float64)
        if self.world > 1:
            v = v / self.world
        return [np.float32(x) for x in v]

    def train(self, Z, X, Y, read_losses=True):
        self._live_only("train")
        b = self.built(int(np.shape(X)[0]))
        self._upload(b, Z, X, Y)
        self.enqueue_train(b)
        return self._read_losses() if read_losses else None

    def run_from_iterator(self, it, Z_sampler, train=True):
        """One train_fn / loss_fn call whose (A, B) batch is produced on the device by a data.Hdf5Iterator
        (uint8 upload + ghm_image_batch straight into the step's input buffers; no fp32 host batch)."""
        self._live_only("run_from_iterator")
        n = it.peek_n()
        b = self.built(n)
        self.sync()
        it.next_into(b.x, b.y)
        b.z.set(np.ascontiguousarray(Z_sampler(n), np.float32))
        self.sync()
        if train:
            self.enqueue_train(b)
        else:
            self._run_loss(b)
        return self._read_losses()

    def _run_loss(self, b):
        self._live_only("loss")
        self._param_ticks += 1                  # loss_fn still updates the BatchNorm running statistics
        if self.use_graph == 'recorded':
            self._run_recorded(b, 'loss')
        else:
            self._run_lanes(b, 'loss', b.loss_prog)
        if self.exchange:
            self._reduce_losses_now()

    def _all_devs(self):
        out = []
        for d in list(self.devs) + [sd[0] for sd in self.side if sd is not None] + [self.cdev]:
            if d is not None and all(d is not o for o in out):
                out.append(d)
        return out

    def _sequence(self, b, name):
        """the host-order launch sequence [(lane, entry)] of a whole call (both stage programs interleaved, then the
        exchange, then the updates)"""
        if name not in b.sequences:
            if name == 'train':
                seq = list(_interleave(b.train_compute[0], b.train_compute[1]))
                seq += [(0, e) for e in b.exchange]
                seq += list(_interleave(b.update[0], b.update[1]))
            else:
                seq = list(_interleave(b.loss_prog[0], b.loss_prog[1]))
            b.sequences[name] = seq
        return b.sequences[name]

    def _run_recorded(self, b, name, wrap=None):
        """call 0 eager (library workspaces take their size), call 1 records the sequence and replays it, later calls
        are ONE ghm_step_run each.  ``wrap(lane, entry)`` at record time brackets entries with recorded timers."""
        self._bind_loss_scale()
        seq = self._sequence(b, name)
        n = b.calls.get(name, 0)
        b.calls[name] = n + 1
        if n == 0:
            for lane, e in seq:
                e[1]()
            return
        if name not in b.steps:
            D = type(self.devs[0])
            st = D.step_record_begin(self._all_devs())
            try:
                for lane, e in seq:
                    if wrap is not None:
                        wrap(lane, e)
                    else:
                        e[1]()
            finally:
                D.step_record_end(st)
            b.steps[name] = st
        type(self.devs[0]).step_run(b.steps[name])

    def enqueue_train(self, b, wrap=None):
        """one train step on the data already resident in b.z / b.x / b.y (asynchronous)"""
        self._live_only("train")
        self._param_ticks += 1
        if self.use_graph == 'recorded':
            return self._run_recorded(b, 'train', wrap)
        if self.exchange:
            self._run_lanes(b, 'train_compute', b.train_compute, wrap)     # eager: bucket all-reduces are inside
            for e in b.exchange:
                e[1]()
            self._run_lanes(b, 'train_update', b.update, wrap)
        else:
            if b.train_all is None:
                b.train_all = [b.train_compute[0] + b.update[0], b.train_compute[1] + b.update[1]]
            self._run_lanes(b, 'train_all', b.train_all, wrap)

    def _reduce_losses_now(self):
        self.sync()
        self.cops.allreduce_sum(self.losses_dev, 8)

    def loss(self, Z, X, Y):
        self._live_only("loss")
        b = self.built(int(np.shape(X)[0]))
        self._upload(b, Z, X, Y)
        self._run_loss(b)
        return self._read_losses()

    def profile_train(self, B):
        """[(label, ms, meta)] per program entry, stream by stream (synchronising; mutates parameters like a
        real step: compute, then the exchange, then the updates)."""
        self._live_only("profile_train")
        self._param_ticks += 1
        b = self.built(B)
        out = []

        def timed(entries, dev, lane):
            for e in entries:
                side = len(e) > 3 and e[3] is not None
                d = e[3] if side else dev
                d.timer_start(1)
                e[1]()
                d.timer_stop(1)
                meta = e[2] if len(e) > 2 else None
                out.append((e[0], d.timer_ms(1), meta, "%s%s" % ("AB"[lane] if lane in (0, 1) else "C", "'" if side else "")))

        for lane in (0, 1):
            timed(b.train_compute[lane], self.devs[lane], lane)
        if self.exchange:
            self.sync()
            timed(b.exchange, self.cdev, 2)
            self.sync()
        for lane in (0, 1):
            timed(b.update[lane], self.devs[lane], lane)
        return out

    # ---- forward-only entry points (pix2pix.py:144-147) -------------------------------------------------
    def _infer_plan(self, key, B, deterministic):
        k = (key, B, deterministic)
        if k not in self._infer:
            lane = LANE_OF[key]
            plan = NetPlan(self.devs[lane], self.ops[lane], self.nets[key], B, self.stores[key], name=key + "_infer",
                           dtype=self.dtype)
            prog = []
            plan.emit_forward(prog, deterministic=deterministic)
            self._infer[k] = (plan, prog)
            self._apply_pending_counters()
        return self._infer[k]

    def _subgraph_plan(self, key, tag, B, build):
        """deterministic forward-only plan of a graph that shares net ``key``'s parameters (terrain.py: the DCGAN generator's
        head, and its trunk re-rooted on a seed canvas); ``build()`` makes the graph's output layer.  Cached per (key, tag, B)
        like _infer_plan, so loading a model or training a step is visible to the next run with nothing re-uploaded."""
        k = (key, tag, B)
        if k not in self._subgraph:
            lane = LANE_OF[key]
            plan = NetPlan(self.devs[lane], self.ops[lane], build(), B, self.stores[key], name="%s_%s" % (key, tag[0]),
                           dtype=self.dtype)
            prog = []
            plan.emit_forward(prog, deterministic=True)
            self._subgraph[k] = (plan, prog)
        return self._subgraph[k]

    def generate(self, key, inp, deterministic=False):
        return self.generate_device(key, inp, deterministic).numpy()

    def generate_device(self, key, inp, deterministic=False):
        """generate() without the download: the forward plan's output DevTensor, enqueued on the net's lane and valid until
        the next forward of the same (net, batch size, deterministic)"""
        if not deterministic:
            self._live_only("a non-deterministic forward (it moves the BatchNorm running statistics)")
        inp = np.ascontiguousarray(inp, np.float32)
        plan, prog = self._infer_plan(key, inp.shape[0], deterministic)
        self._param_ticks += not deterministic  # batch statistics move the running ones
        self.sync()
        plan.input_nodes[0].out.set(inp)
        for e in prog:
            e[1]()
        return plan.out

    def generate_chain(self, Z, deterministic=True):
        """z -> G(z) -> U(G(z)) without leaving HBM (the z_fn -> gen_fn chain of generate_interpolation_clip,
        /root/reference/pix2pix.py:384-393).  Returns (heightmaps, textures) as numpy arrays."""
        if not deterministic:
            self._live_only("a non-deterministic forward (it moves the BatchNorm running statistics)")
        Z = np.ascontiguousarray(Z, np.float32)
        pg, prog_g = self._infer_plan('dcgan_gen', Z.shape[0], deterministic)
        pu, prog_u = self._infer_plan('p2p_gen', Z.shape[0], deterministic)
        self._param_ticks += not deterministic
        self.sync()
        pg.input_nodes[0].out.set(Z)
        for e in prog_g:
            e[1]()
        lg, lu = LANE_OF['dcgan_gen'], LANE_OF['p2p_gen']
        if self.devs[lu] is not self.devs[lg]:
            self.devs[lu].wait_for(self.devs[lg])
        self.ops[lu].copy_view(pg.out, pu.input_nodes[0].out)
        for e in prog_u:
            e[1]()
        a = pg.out.numpy()
        return a, pu.out.numpy()

