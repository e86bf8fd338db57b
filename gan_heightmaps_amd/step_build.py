"""Builds the plan set of one batch size for step.GanStep: the four NetPlans wired into each other, the loss and train
programs of the two stage streams, the data-parallel exchange and the update lists.  The ORDER of the device allocations and
of the entries appended here is the memory layout and the launch sequence of the step (tools/lowering_trace.py pins both)."""
import os

import numpy as np

from . import layers as L
from .engine import NetPlan

LANE_OF = {'dcgan_gen': 0, 'dcgan_disc': 0, 'p2p_gen': 1, 'p2p_disc': 1}
EMA_NETS = ('dcgan_gen', 'p2p_gen')        # the nets inference runs: only they keep an average (GanStep(ema=decay))


def _has_bn(layer):
    return any(isinstance(l, L.BatchNormLayer) for l in L.get_all_layers(layer))


def _input_layer(net):
    return [l for l in L.get_all_layers(net) if isinstance(l, L.InputLayer)][0]


class _Built:
    """the plan set of one (batch size, slot): what StepBuilder.build returns and GanStep issues"""

    def __init__(self, B):
        self.B = B                          # batch size
        self.G = self.D = None              # NetPlans of the DCGAN stage: generator (B samples), discriminator (2B: real | fake)
        self.U = self.P = None              # NetPlans of the pix2pix stage: U-Net (B), PatchGAN (2B)
        self.d_in = None                    # D's input batch: X in the first half, G(z) written into the second
        self.z = self.x = self.y = None     # the step's inputs: latent vectors, heightmaps X, textures Y
        self.seed_D = self.seed_G = None    # loss-gradient seeds of the DCGAN stage (discriminator loss on 2B, generator loss on B)
        self.seed_PD = self.seed_PG = None  # the same of the pix2pix stage
        self.seed_Df = None                 # fake half of seed_D kept aside (rank-one shortcut only)
        self.loss_prog = None               # [stream A, stream B] entries of loss_fn: forward + losses
        self.train_compute = None           # [stream A, stream B] entries of train_fn up to the gradients
        self.exchange = []                  # entries behind both stage programs: collectives, sharded updates, waits
        self.update = [[], []]              # [stream A, stream B] optimiser entries
        self.xchg_order = []                # [(label, net key, first element, n elements)] in collective order
        self.net_buckets = {}               # {net key: [(lo, hi)]} sub-buckets of the flat gradient buffer, in completion order
        self.graphs = {}                    # {program name: [captured graph per stream]} (use_graph=True)
        self.calls = {}                     # {program name: times issued} (the first call is always eager)
        self.steps = {}                     # {program name: library step handle} (captured graphs / recorded sequence)
        self.sequences = {}                 # {'train' / 'loss': [(lane, entry)]} host-order launch sequences (GanStep._sequence)
        self.train_all = None               # [stream A, stream B] train_compute + update (no exchange), made at first issue


def cut_buckets(offsets, sizes, n_train, n_pad, bucket_bytes, unit, sharded):
    """A net's flat gradient range as SUB-BUCKETS: contiguous ranges of >= bucket_bytes each, cut in the order the backward pass
    completes them (last layers first = highest offsets first).  ``offsets`` / ``sizes``: the trainable parameters, ascending.
    -> [(lo, hi, pending)] with ``pending`` the indices of the parameters whose gradients the range holds."""
    offs = list(offsets) + [n_train]
    buckets, hi, pend = [], (n_pad if sharded else n_train), []
    for i in range(len(offsets) - 1, -1, -1):
        pend.append(i)
        # sharded form: a bucket starts on a multiple of world x 64 elements (world equal, line-aligned shards); the
        # parameter that straddles the cut belongs to BOTH neighbours' pending sets (it completes last anyway)
        lo = offs[i] // unit * unit if i else 0
        if (4 * (hi - lo) >= bucket_bytes and lo < hi) or i == 0:
            straddle = [q for q in range(i) if offsets[q] + sizes[q] > lo] if lo < offs[i] else []
            if hi > lo:
                buckets.append((lo, hi, set(pend + straddle)))
            hi, pend = lo, list(straddle)
    return buckets


class BucketSender:
    """the sub-buckets of one net while its backward pass is emitted: ``send(index, lo, hi)`` is called for a bucket when the
    launch that completes its last gradient has been reported (on_grads is emit_backward's hook), so only the final one (the
    first layers' few parameters) is exposed behind the stage's last kernel; the rest travels under the remaining backward
    pass"""

    def __init__(self, buckets, params, send):
        self.buckets, self.send = buckets, send
        self.pending = [{id(params[i]) for i in pend} for _, _, pend in buckets]
        self.sent = [False] * len(buckets)
        self.of = {}                    # id(parameter) -> the buckets that wait for it
        for i, pend in enumerate(self.pending):
            for pid in pend:
                self.of.setdefault(pid, []).append(i)

    def _send(self, i):
        self.sent[i] = True
        self.send(i, self.buckets[i][0], self.buckets[i][1])

    def on_grads(self, _prog, params):
        for p in params:
            for i in self.of.get(id(p), ()):
                self.pending[i].discard(id(p))
                if not self.pending[i] and not self.sent[i]:
                    self._send(i)

    def flush(self):                # parameters no launch reported (none today): their bucket still travels
        for i in range(len(self.buckets)):
            if not self.sent[i]:
                self._send(i)


class StepBuilder:
    """one use: StepBuilder(engine, B).build().  The fields are what the parts share."""

    def __init__(self, eng, B):
        self.eng, self.B, self.b = eng, B, _Built(B)
        self.dA, self.dB = eng.devs
        self.oA, self.oB = eng.ops
        self.cdev, self.cops = eng.cdev, eng.cops
        self.slot = lambda i: eng.losses_dev.channels(i, i + 1)
        self.l2 = eng.reconstruction == 'l2'
        self.LS = 1.0               # the fp16 loss scale is device state read by the loss kernels (ghm_set_loss_scale_state)
        self.do_dcgan = eng.train_mode in ('both', 'dcgan')
        self.do_p2p = eng.train_mode in ('both', 'p2p')
        self.tdone = set()          # conv weights whose transposed copy is already fresh in this program
        self.embed = eng.exchange and eng.use_graph is not True  # RCCL calls stay outside captured HIP graphs
        self.late = []              # graph mode: the collectives stay outside the captured graphs, after both programs
        # sharded update: a net's parameters are all-gathered at the END of a step in forward order (G, U, D, P; within a net the
        # first layers first) and the NEXT step's forward waits per net, right in front of the net's first weight read -- the
        # discriminators' gathers run under the generators' forward passes instead of in front of the whole step
        # (captured HIP graphs, use_graph=True: an event wait cannot sit inside a capture -- ghm_event_wait refuses -- so that
        # form keeps one wait for the communication stream at the end of the step, as the all-reduce form does)
        self.per_net_waits = eng.sharded and eng.use_graph is not True
        self.gev = {}               # {net key: event behind its last gather} (per_net_waits)

    def build(self):
        b, eng = self.b, self.eng
        self.plans()
        fa, fb = self.forward()
        # ---- loss_fn (:143): forward + losses, BN running stats still update ----
        la, lb = list(fa), list(fb)
        self.losses(la, 0, False)
        self.losses(lb, 1, False)
        lb.append(("recon", lambda: self.oB.recon_loss(b.U.out, b.y, self.slot(3), None, 1.0, self.l2)))
        b.loss_prog = [la, lb]
        # ---- train_fn (:142) ----
        ta, tb = list(fa), list(fb)
        self.losses(ta, 0, True)
        self.losses(tb, 1, True)
        if self.do_dcgan:
            self.stage_backward(ta, 0)
        if self.do_p2p:
            self.stage_backward(tb, 1)
        else:
            tb.append(("recon", lambda: self.oB.recon_loss(b.U.out, b.y, self.slot(3), None, 1.0, self.l2)))
        if eng.side[0] is not None:        # the gradient streams rejoin before anything consumes the gradients
            ta.append(("join", lambda: self.dA.wait_for(eng.side[0][0])))
            tb.append(("join", lambda: self.dB.wait_for(eng.side[1][0])))
        b.train_compute = [ta, tb]
        # ---- after both stage programs: (graph mode: the bucket all-reduces, in a fixed order), the losses, then
        # the stage streams wait for the communication stream and apply their own nets' updates (:131-141) ----
        self.keys = (['dcgan_gen', 'dcgan_disc'] if self.do_dcgan else []) + (['p2p_gen', 'p2p_disc'] if self.do_p2p else [])
        if eng.exchange:
            self.exchange_tail()
        self.updates()
        return b

    # ---- plans and input wiring ----
    def plans(self):
        b, eng, B, dA, dB, oA, oB = self.b, self.eng, self.B, self.dA, self.dB, self.oA, self.oB
        # dropout step counters live per (net, batch size) on the engine, whichever slot of that batch size is built first: both
        # slots of a batch size advance ONE counter, so the pipelined loop draws the masks of the sequential loop (a ragged last
        # batch first seen on an odd step builds slot 1 before slot 0)
        rc = eng._rng_counters
        G, D, U, P = (eng.nets[k] for k in ('dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc'))
        self.d_in_layer, u_in_layer = _input_layer(D), _input_layer(U)
        i_a, self.i_b = eng.p2p_disc_inputs
        ca, H, W = self.d_in_layer.shape[1:]
        b.d_in = dA.empty((2 * B, ca, H, W))
        # which nets fork their weight / bias gradients onto the gradient stream: all but the DCGAN generator, whose
        # small weight gradients stay inline on stage A (measured img/s, fp32 / bf16 / fp32 batch 2 / 1024^2 fp16:
        # DPU 169.4 / 492.3 / 153.0 / 98.9, PU 169.3 / 498.8 / 150.5 / 97.2, GDPU 167.7 / 471.9 / 150.4 / 97.2,
        # none 164.5 / 467.1, GD 164.0).  GHM_SIDE_NETS overrides (tuning).
        # (reduced precision: +1 % with D inline too; the split-fp32 mode, whose kernels are as long as the fp32 ones: 253 -> 261 img/s with D on the side)
        _sn = os.environ.get('GHM_SIDE_NETS', 'DPU' if eng.dtype in ('f32', 'bf16x3', 'bf16x2') else 'PU')
        _side = lambda k, lane: eng.side[lane] if k in _sn else None
        b.G = NetPlan(dA, oA, G, B, eng.stores['dcgan_gen'], out_tensor=b.d_in.samples(B, 2 * B), name="G",
                      side=_side('G', 0), rng_seed=eng.rank, dtype=eng.dtype,       # replicas draw different dropout masks
                      rng_counter=rc.get(('G', B)))
        b.D = NetPlan(dA, oA, D, 2 * B, eng.stores['dcgan_disc'], inputs={self.d_in_layer: b.d_in}, name="D",
                      side=_side('D', 0), bn_groups=2 if _has_bn(D) else 1, dtype=eng.dtype)
        b.P = NetPlan(dB, oB, P, 2 * B, eng.stores['p2p_disc'], name="P", side=_side('P', 1),
                      bn_groups=2 if _has_bn(P) else 1, dtype=eng.dtype)
        self.pa, self.pb = b.P.input_tensor(i_a), b.P.input_tensor(self.i_b)
        b.U = NetPlan(dB, oB, U, B, eng.stores['p2p_gen'], out_tensor=self.pb.samples(B, 2 * B), name="U",
                      side=_side('U', 1), rng_seed=eng.rank, dtype=eng.dtype,
                      rng_counter=rc.get(('U', B)))
        rc.setdefault(('G', B), b.G.rng_counter)
        rc.setdefault(('U', B), b.U.rng_counter)
        eng._apply_pending_counters()
        b.z = b.G.input_nodes[0].out
        b.x = b.U.input_tensor(u_in_layer)
        b.y = dB.empty((B,) + tuple(self.pb.shape[1:]))

    # ---- shared forward (pix2pix.py:92-101), one list per stream ----
    def gwait(self, prog, dev_, k):
        if k in self.gev:
            prog.append(("wait_gather_" + k, lambda ev=self.gev[k]: dev_.event_wait(ev), None, dev_))

    def forward(self):
        b, eng, B, dA, dB, oA, oB, pa, pb = self.b, self.eng, self.B, self.dA, self.dB, self.oA, self.oB, self.pa, self.pb
        if self.per_net_waits:
            self.gev = eng._gather_events()
        fa = [("x_to_d_in", lambda: oA.copy_view(b.x, b.d_in.samples(0, B)))]
        fb = []
        if self.per_net_waits:
            # nothing waits for the communication stream at the end of a sharded step, and a stage whose nets were not
            # exchanged (train_mode 'dcgan' / 'p2p') never meets a gather event: its loss kernels of the NEXT step write
            # losses_dev, which the previous step's loss all-reduce may still be reading -- both stage streams wait for the
            # event recorded behind that all-reduce (unrecorded on the first step: the wait is a no-op)
            lev = eng._losses_event()
            fa.append(("wait_losses_reduced", lambda: dA.event_wait(lev), None, dA))
            if dB is not dA:
                fb.append(("wait_losses_reduced", lambda: dB.event_wait(lev), None, dB))
        self.gwait(fa, dA, 'dcgan_gen')
        b.G.emit_forward(fa)
        self.gwait(fa, dA, 'dcgan_disc')
        b.D.emit_forward(fa)
        fb += [("x_to_p_in0", lambda: oB.copy_view(b.x, pa.samples(0, B))),
               ("x_to_p_in1", lambda: oB.copy_view(b.x, pa.samples(B, 2 * B))),
               ("y_to_p_in", lambda: oB.copy_view(b.y, pb.samples(0, B)))]
        self.gwait(fb, dB, 'p2p_gen')
        b.U.emit_forward(fb)
        self.gwait(fb, dB, 'p2p_disc')
        b.P.emit_forward(fb)
        d_out, p_out = b.D.out, b.P.out
        b.seed_D, b.seed_G = dA.empty(d_out.shape), dA.empty(d_out.samples(B, 2 * B).shape)
        b.seed_PD, b.seed_PG = dB.empty(p_out.shape), dB.empty(p_out.samples(B, 2 * B).shape)
        return fa, fb

    def losses(self, prog, lane, g):
        """the three adversarial-loss entries of a stage; ``g``: they also write the loss-gradient seeds (train_fn)
        stage A: (:107) gen_loss_dcgan, (:108) disc_loss_dcgan; stage B: (:110) gen_loss_p2p, (:121) disc_loss_p2p"""
        b, B, LS, slot = self.b, self.B, self.LS, self.slot
        o = self.eng.ops[lane]
        adv = o.lsgan_loss if self.eng.lsgan else o.bce_loss
        out, seed_g, seed_d, sg, sd = ((b.D.out, b.seed_G, b.seed_D, 0, 1), (b.P.out, b.seed_PG, b.seed_PD, 2, 4))[lane]
        real, fake = out.samples(0, B), out.samples(B, 2 * B)
        prog.append(("loss", lambda: adv(fake, 1.0, slot(sg), seed_g if g else None, LS)))
        prog.append(("loss", lambda: adv(real, 1.0, slot(sd), seed_d.samples(0, B) if g else None, LS)))
        prog.append(("loss", lambda: adv(fake, 0.0, slot(sd), seed_d.samples(B, 2 * B) if g else None,
                                         LS, True)))

    # ---- data-parallel exchange (no reference counterpart) ----
    # One all-reduce per net bucket on the COMMUNICATION stream (the communicator's context), enqueued where the
    # bucket's last gradient kernel has been issued: the discriminator buckets reduce under the generator's
    # backward pass, the DCGAN buckets under the pix2pix stage.  The communication stream waits for the streams
    # that wrote the bucket (events recorded at this point of the program), the collectives run in host-enqueue
    # order, and that order is a pure function of the program -- identical on every rank.
    def bucket_hook(self, k, lane, prog):
        """-> (on_grads callback for emit_backward, flush) that put the collectives of net ``k``'s sub-buckets into ``prog``
        (embedded form) or behind both programs (captured graphs); (None, no-op) without an exchange"""
        eng, b, cdev, cops = self.eng, self.b, self.cdev, self.cops
        if not eng.exchange:
            return None, lambda: None
        st = eng.stores[k]
        srcs = [eng.devs[lane]] + ([eng.side[lane][0]] if eng.side[lane] is not None else [])
        tr = sorted((p for p in st.params if p.index[0] == 'w'), key=lambda p: p.index[1])
        buckets = cut_buckets([p.index[1] for p in tr], [int(np.prod(p.shape)) for p in tr], st.n_train, st.n_pad,
                              eng.bucket_bytes, eng.shard_unit, eng.sharded)
        b.net_buckets[k] = [(lo, hi) for lo, hi, _ in buckets]
        half = eng.exchange_mode == 'allreduce_bf16'
        if half and k not in eng.xchg_bf16:
            eng.xchg_bf16[k] = cdev.alloc(2 * st.n_pad + 256)          # the net's bf16 exchange buffer (one halfword per gradient)
        sharded, world = eng.sharded, eng.world

        def send(i, lo, hi):
            n = hi - lo
            view = st.g.channels(lo, hi)
            label = ("reducescatter_" if sharded else "allreduce_") + ("%s_%d" % (k, i) if len(buckets) > 1 else k)

            def fn():
                for d in srcs:
                    cdev.wait_for(d)
                if sharded:
                    cops.reduce_scatter_sum(view, n // world)
                elif half:
                    cops.allreduce_sum_bf16(view, n, eng.xchg_bf16[k] + 2 * lo)
                else:
                    cops.allreduce_sum(view, n)
            b.xchg_order.append((label, k, lo, n))
            (prog if self.embed else self.late).append((label, fn, None, cdev))
        sender = BucketSender(buckets, tr, send)
        return sender.on_grads, sender.flush

    def stage_backward(self, prog, lane):
        """the backward passes of one stage, all at the pre-update parameters: discriminator loss through the discriminator
        (weights + data gradients, 2B batch), generator loss through it on the fake half (data gradients only), then through
        the generator.  Stage A may take the second from the first (rank-one shortcut); stage B adds the reconstruction term."""
        b, B, tdone = self.b, self.B, self.tdone
        dev, o = self.eng.devs[lane], self.eng.ops[lane]
        disc, gen, kd, kg, seed_d, seed_g, in_layer = (
            (b.D, b.G, 'dcgan_disc', 'dcgan_gen', b.seed_D, b.seed_G, self.d_in_layer),
            (b.P, b.U, 'p2p_disc', 'p2p_gen', b.seed_PD, b.seed_PG, self.i_b))[lane]
        disc.emit_transposes(prog, tdone)
        gen.emit_transposes(prog, tdone)
        hook, flush = self.bucket_hook(kd, lane, prog)
        n1 = self.eng._per_sample_scalar_head(disc, in_layer, self.eng.dtype) if lane == 0 else None
        if n1 is not None:
            # the fake half of the discriminator-loss seed, kept aside (a backward pass may modify its seed in place)
            b.seed_Df = dev.empty(seed_g.shape)
            prog.append(("seed_copy", lambda: o.copy_view(seed_d.samples(B, 2 * B), b.seed_Df)))
        disc.emit_backward(prog, seed_d, wgrad=True, tag="dloss", transposed=tdone, on_grads=hook)
        flush()
        if n1 is not None:
            # D returns ONE scalar per sample and no layer couples samples: its backward pass on sample n is linear in
            # the single number dLoss/dD(G(z))_n, so the generator-loss gradient at every depth is the discriminator-loss
            # gradient of the fake half times seed_G[n] / seed_D[n].  The dloss pass above already walked the fake half
            # down to the first layer's output; only that layer's data gradient is left, then one per-sample factor
            # (:107-108: both losses read the same D(G(z)); 12 -> 8 image-backward passes through D per step).
            g1 = disc.grads_of(n1).samples(B, 2 * B)
            gin = disc.emit_backward(prog, None, nslice=(B, 2 * B), wgrad=False, input_grads=[in_layer],
                                     tag="gloss", transposed=tdone, resume={n1: g1})
            gfake = gin[in_layer]
            prog.append(("per_sample_ratio", lambda: o.scale_samples(gfake, seed_g, b.seed_Df)))
        else:
            gin = disc.emit_backward(prog, seed_g, nslice=(B, 2 * B), wgrad=False, input_grads=[in_layer],
                                     tag="gloss", transposed=tdone)
        gu = gin[in_layer]
        if lane == 1:
            # (:115-117) recon loss and alpha * d recon / d U(X) added to the adversarial gradient
            prog.append(("recon", lambda: o.recon_loss(b.U.out, b.y, self.slot(3), gu, self.eng.alpha * self.LS, self.l2, True)))
        hook, flush = self.bucket_hook(kg, lane, prog)
        gen.emit_backward(prog, gu, wgrad=True, transposed=tdone, on_grads=hook)
        flush()

    def exchange_tail(self):
        """behind both stage programs, on the communication stream: (captured graphs: every sub-bucket's collective), the loss
        all-reduce, (sharded form: the shard updates and the gathers), then the stage streams' waits"""
        b, eng, dA, dB, cdev, cops = self.b, self.eng, self.dA, self.dB, self.cdev, self.cops
        b.exchange.extend(self.late)          # graph mode: every sub-bucket, in completion order per stage

        def reduce_losses():
            cdev.wait_for(dA)
            if dB is not dA:
                cdev.wait_for(dB)
            cops.allreduce_sum(eng.losses_dev, 8)
        b.exchange.append(("allreduce_losses", reduce_losses, None, cdev))
        if self.per_net_waits:
            b.exchange.append(("losses_reduced", lambda ev=eng._losses_event(): cdev.event_record(ev), None, cdev))
        if eng.sharded:
            self.sharded_updates()
        # one entry per stage stream, so that bench.py can bracket each with HIP events: the time a stage stream
        # spends in this wait is the EXPOSED part of the exchange
        # (sharded form: no wait here -- the next forward waits per net, ``wait_gather_*`` above; except under captured
        # HIP graphs, where the waits cannot sit inside the graphs)
        if not self.per_net_waits:
            b.exchange.append(("wait_comm", lambda: dA.wait_for(cdev), None, dA))
            if dB is not dA:
                b.exchange.append(("wait_comm", lambda: dB.wait_for(cdev), None, dB))

    def sharded_updates(self):
        b, eng, cdev, cops, gev = self.b, self.eng, self.cdev, self.cops, self.gev
        # (the communication stream has just waited for both stage streams: every kernel that reads the pre-update
        # weights is behind it.)  Per sub-bucket, in the order it was reduced: this rank's shard of the optimiser
        # update, then the all-gather of the updated parameter shards.
        gs_, hp_, kind, rule = 1.0 / eng.world, eng.opt_spec.hp, eng.opt_spec.kind, eng.opt_rule
        # forward order: the nets as the next step reads them (the generators of both stages first), a net's
        # sub-buckets by ascending offset = first layers first; a per-net event behind its last gather
        fwd_rank = {'dcgan_gen': 0, 'p2p_gen': 1, 'dcgan_disc': 2, 'p2p_disc': 3}
        order = sorted(b.xchg_order, key=lambda t: (fwd_rank[t[1]], t[2]))
        last_of = {t[1]: i for i, t in enumerate(order)}
        for idx, (label, k, blo, n) in enumerate(order):
            st, hy, sh = eng.stores[k], eng.hyper[k], n // eng.world
            a0 = blo + eng.rank * sh
            wv, gv = st.w.channels(a0, a0 + sh), st.g.channels(a0, a0 + sh)
            sv = [st.opt_state[s].channels(a0, a0 + sh) for s in rule.slots]
            b.exchange.append((kind + "_shard_" + label, lambda wv=wv, gv=gv, sv=sv, hy=hy, sh=sh: rule.run(
                cops, wv, gv, sv, sh, hy, hp_, gs_), None, cdev))
            full = st.w.channels(blo, blo + n)
            b.exchange.append(("allgather_" + label[len("reducescatter_"):], lambda full=full, sh=sh: cops.all_gather(full, sh),
                               None, cdev))
            if last_of[k] == idx and k in gev:
                b.exchange.append(("gathered_" + k, lambda ev=gev[k]: cdev.event_record(ev), None, cdev))
        if rule.ticks:
            for k in self.keys:
                b.exchange.append((kind + "_tick_" + k, lambda hy=eng.hyper[k]: cops.adam_tick(hy), None, cdev))

    def updates(self):
        b, eng, keys = self.b, self.eng, self.keys
        gs = 1.0 / eng.world          # (x 1 / loss scale inside the optimiser kernels, from the device state)
        hp, kind, rule = eng.opt_spec.hp, eng.opt_spec.kind, eng.opt_rule
        # one stream for both stages: one update list, so the fp16 sequence check* -> update* -> scale update is kept
        ulane = (lambda k: 0) if (eng._ls_state and eng.devs[1] is eng.devs[0]) else (lambda k: LANE_OF[k])
        if eng._ls_state:
            # fp16: every gradient bucket of the stage is checked (after its all-reduce: all ranks see the same sum, so
            # they skip or apply together) before the first update of the stage reads the flag
            for k in keys:
                st, lane = eng.stores[k], ulane(k)
                b.update[lane].append(("grad_check_" + k, lambda st=st, o=eng.ops[lane]: o.grad_check(st.g, st.n_train)))
        for k in ([] if eng.sharded else keys):       # (sharded form: the updates ran on the communication stream, above)
            st, hy = eng.stores[k], eng.hyper[k]
            lane = ulane(k)
            o = eng.ops[lane]
            sv = [st.opt_state[s] for s in rule.slots]
            b.update[lane].append((kind + "_" + k, lambda st=st, sv=sv, hy=hy, o=o: rule.run(
                o, st.w, st.g, sv, st.n_train, hy, hp, gs)))
            if rule.ticks:
                b.update[lane].append((kind + "_tick_" + k, lambda hy=hy, o=o: o.adam_tick(hy)))
            if eng.ema is not None and k in EMA_NETS:
                # the generator's average follows its update on the same stream; in fp16 it reads the same
                # overflow flag, so it stands before loss_scale_update clears it
                b.update[lane].append(("ema_" + k, lambda st=st, o=o: o.ema_update(st.ema, st.w, st.n_train, eng.ema)))
        if eng._ls_state:
            for lane in (0, 1):
                if b.update[lane]:
                    b.update[lane].append(("loss_scale_update", lambda o=eng.ops[lane]: o.loss_scale_update(
                        eng.ls_growth_interval, eng.ls_min, eng.ls_max)))
