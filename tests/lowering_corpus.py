"""A deterministic corpus of small layer graphs for the engine's lowering (engine.NetPlan), and the runner that holds one
graph on a device to the float64 layer-graph interpreter (tests/golden/symtheano.py on the oracle's ops).

Two kinds of graphs:
  * NAMED graphs, each aimed at one rewrite / placement / kernel-family decision of engine.py on both sides of its
    threshold (R1 act(concat) split + sharing, R2 epilogue folding, R3 / R3b collapsed up-sample convolutions, fused
    conv + max-pool, the q-copy placement of concat slices, fused conv + BatchNorm, thin and small-map layers, ...);
  * GENERATED graphs from a small grammar over the same layer vocabulary, one fixed np.random.RandomState seed each.

Every graph is small (batch 1-4, maps up to 64 x 64) so that the interpreter stays cheap.  ``graph(name)`` builds a graph
afresh (same parameters every time: the initialiser's RNG is seeded per graph).
"""
import os
import sys

import numpy as np

from gan_heightmaps_amd import init as INIT, layers as L
from gan_heightmaps_amd.architectures import p2p
from gan_heightmaps_amd.architectures.layers import BilinearUpsample2DLayer
from gan_heightmaps_amd.nonlinearities import LeakyRectify, leaky_rectify, linear, rectify, sigmoid, tanh

MODES = ('f32', 'bf16x3', 'bf16x2', 'bf16', 'f16')

LRELU = LeakyRectify(0.2)


class Graph:
    """out: the output layer; inputs: its InputLayers in feed order; feeds: one fp32 array per input; bn_groups: NetPlan's"""

    def __init__(self, name, out, inputs, feeds, bn_groups=1):
        self.name, self.out, self.inputs, self.bn_groups = name, out, list(inputs), bn_groups
        self.feeds = [np.asarray(f, np.float32) for f in feeds]
        self.batch = self.feeds[0].shape[0]


def _inp(rng, shape, positive=False):
    layer = L.InputLayer((None,) + tuple(shape[1:]))
    x = rng.rand(*shape) if positive else rng.randn(*shape)
    return layer, x


def _conv(x, k_out, k, stride=1, pad='same', act=linear):
    return L.Conv2DLayer(x, k_out, k, stride=stride, pad=pad, nonlinearity=act)


def _bn(x, act=None):
    y = L.BatchNormLayer(x)
    return y if act is None else L.NonlinearityLayer(y, act)


def _chain(name, rng, shape, body, positive=False, bn_groups=1):
    i, x = _inp(rng, shape, positive)
    return Graph(name, body(i), [i], [x], bn_groups)


# ---- named graphs --------------------------------------------------------------------------------------------------
def _up_nearest_conv5(rng):          # R3 mode 0, with a BatchNorm behind (bn_apply_hi) and a plain lrelu epilogue
    return _chain("up_nearest_conv5", rng, (2, 16, 32, 32),
                  lambda i: _bn(_conv(L.Upscale2DLayer(i, 2), 32, 5), rectify))


def _up_nearest_conv5_act(rng):
    return _chain("up_nearest_conv5_act", rng, (2, 8, 16, 16),
                  lambda i: _conv(L.Upscale2DLayer(i, 2), 16, 5, act=LRELU))


def _blconv(name, shape, k_out, tail):
    def build(rng):
        return _chain(name, rng, shape, lambda i: tail(_conv(BilinearUpsample2DLayer(i, 2), k_out, 3, pad=1)))
    return build


def _blconv_act(name, act):
    def build(rng):                  # the nonlinearity on the conv itself
        return _chain(name, rng, (2, 32, 32, 32), lambda i: _conv(BilinearUpsample2DLayer(i, 2), 32, 3, pad=1, act=act))
    return build


def _convpool(name, shape, k_out, k, act, separate=False):
    def body(i):
        c = _conv(i, k_out, k, act=linear if separate else act)
        if separate:
            c = L.NonlinearityLayer(c, act)
        p = L.MaxPool2DLayer(c, 2)
        return _conv(p, 8, 3, act=linear)
    return lambda rng: _chain(name, rng, shape, body)


def _conv_bn_act(rng):               # conv -> BN -> act twice; the second pair on a 16 x 16 map
    def body(i):
        x = _bn(_conv(i, 32, 3), LRELU)
        x = _bn(_conv(x, 32, 3, stride=2, pad=1), rectify)
        return _conv(x, 8, 3)
    return _chain("conv_bn_act", rng, (2, 16, 32, 32), body)


def _conv_bn_act_small(rng):         # conv -> BN -> act on small maps (the finishing kernel holds the whole map)
    return _chain("conv_bn_act_small", rng, (2, 32, 16, 16),
                  lambda i: _conv(_bn(_conv(i, 32, 3), LRELU), 16, 3))


def _conv_act_bn(rng):               # conv -> act -> BN: pixel_discriminator(bn=True)'s placement
    def body(i):
        x = L.BatchNormLayer(L.NonlinearityLayer(_conv(i, 32, 3), leaky_rectify))
        return _conv(x, 1, 3, act=sigmoid)
    return _chain("conv_act_bn", rng, (2, 16, 32, 32), body)


def _pixel_discriminator_bn(rng):
    d = p2p.pixel_discriminator(16, True, False, nf=8, act=linear, bn=True)
    a, b = rng.rand(2, 1, 16, 16), rng.randn(2, 3, 16, 16)
    return Graph("pixel_discriminator_bn", d["out"], d["inputs"], [a, b])


def _unet_skip(rng):
    """the U-Net skip pattern: the encoder applies leaky_rectify to a, the decoder to concat(up, a) -> R1 splits the act
    over the concat and shares the encoder's act(a)"""
    i, x = _inp(rng, (2, 8, 32, 32))
    a = _conv(i, 16, 3, stride=2, pad=1)                         # 16 x 16
    ea = L.NonlinearityLayer(a, leaky_rectify)
    b = _bn(_conv(ea, 32, 3, stride=2, pad=1))                  # 8 x 8
    up = _bn(L.Deconv2DLayer(L.NonlinearityLayer(b, leaky_rectify), 16, 2, stride=2, nonlinearity=linear))
    cat = L.NonlinearityLayer(L.ConcatLayer([up, a]), leaky_rectify)
    out = _conv(cat, 8, 3, pad=1, act=tanh)
    return Graph("unet_skip", out, [i], [x])


def _concat(name, widths, k_out=32):
    def build(rng):
        i, x = _inp(rng, (2, 8, 32, 32))
        parts = [_conv(i, w, 3, act=LRELU) for w in widths]
        return Graph(name, _conv(L.ConcatLayer(parts), k_out, 3), [i], [x])
    return build


def _concat_input_slice(rng):        # a net input written in place into a concat buffer beside a conv output
    i, x = _inp(rng, (2, 8, 32, 32))
    c = _conv(i, 24, 3, act=rectify)
    return Graph("concat_input_slice", _conv(L.ConcatLayer([c, i]), 32, 3), [i], [x])


def _stride2_odd(rng):
    def body(i):
        x = _conv(i, 16, 3, stride=2, pad=1, act=LRELU)            # 17 x 23 -> 9 x 12
        x = _conv(x, 16, 3, stride=2, pad=1, act=rectify)          # -> 5 x 6
        return _conv(x, 4, 3, stride=2, pad=1)                     # -> 3 x 3
    return _chain("stride2_odd", rng, (2, 8, 17, 23), body)


def _stride2_5x5_rect(rng):
    return _chain("stride2_5x5_rect", rng, (2, 16, 33, 64),
                  lambda i: _conv(_conv(i, 32, 5, stride=2, pad=2, act=LRELU), 16, 3, stride=2, pad=1))


def _small_maps(rng):                # 8 x 8 -> 4 x 4 -> 2 x 2 -> a 2 x 2 filter -> 1 x 1
    def body(i):
        x = _bn(_conv(i, 32, 3), LRELU)
        x = _conv(x, 32, 3, stride=2, pad=1, act=rectify)
        x = _conv(x, 16, 3, stride=2, pad=1, act=LRELU)
        return _conv(x, 8, 2, pad=0)
    return _chain("small_maps", rng, (3, 32, 8, 8), body)


def _tiny_2x2(rng):
    return _chain("tiny_2x2", rng, (4, 16, 2, 2), lambda i: _conv(_conv(i, 32, 3, act=LRELU), 8, 2, pad=0, act=tanh))


def _one_filter_out(rng):
    return _chain("one_filter_out", rng, (2, 16, 32, 32), lambda i: _conv(_conv(i, 32, 3, act=LRELU), 1, 3, act=sigmoid))


def _one_filter_5x5(rng):
    return _chain("one_filter_5x5", rng, (2, 3, 32, 32), lambda i: _conv(_conv(i, 8, 5, act=rectify), 1, 5), positive=True)


def _deconv(rng):
    def body(i):
        x = _bn(L.Deconv2DLayer(i, 16, 2, stride=2, nonlinearity=linear), rectify)      # 8 -> 16
        x = L.Deconv2DLayer(x, 16, 2, stride=1, nonlinearity=LRELU)                      # 16 -> 17
        return L.Deconv2DLayer(x, 4, 2, stride=2, nonlinearity=tanh)                     # 17 -> 34
    return _chain("deconv", rng, (2, 16, 8, 8), body)


def _dcgan_head(rng):                # Dense -> Reshape -> BN -> relu -> nearest x2 -> 5x5 conv (dcgan.py's generator head)
    i = L.InputLayer((None, 20))
    x = L.DenseLayer(i, 16 * 4 * 4, nonlinearity=linear)
    x = _bn(L.ReshapeLayer(x, (-1, 16, 4, 4)), rectify)
    x = _bn(_conv(L.Upscale2DLayer(x, 2), 16, 5), rectify)
    out = _conv(L.Upscale2DLayer(x, 2), 1, 5, act=tanh)
    return Graph("dcgan_head", out, [i], [rng.rand(3, 20)])


def _dense_tail(rng):                # conv -> flattening dense (the discriminator's output layer)
    return _chain("dense_tail", rng, (2, 8, 8, 8),
                  lambda i: L.DenseLayer(_conv(i, 16, 3, stride=2, pad=1, act=LRELU), 1, nonlinearity=sigmoid))


def _instance_norm(rng):
    def body(i):
        x = L.NonlinearityLayer(L.InstanceNormLayer(_conv(i, 16, 3)), LRELU)
        return L.InstanceNormLayer(_conv(x, 8, 3))
    return _chain("instance_norm", rng, (2, 8, 16, 16), body)


def _dropout(rng):
    return _chain("dropout", rng, (2, 8, 16, 16),
                  lambda i: _conv(L.DropoutLayer(_conv(i, 16, 3, act=rectify), p=0.3), 8, 3))


def _avgpool(name, p):
    return lambda rng: _chain(name, rng, (2, 8, 32, 32),
                              lambda i: _conv(L.Pool2DLayer(_conv(i, 16, 3, act=LRELU), p, mode='average_inc_pad'), 8, 3))


def _patchgan(rng):
    d = p2p.discriminator(32, True, False, nf=8, act=sigmoid, mul_factor=[1, 2], bn=True)
    a, b = rng.rand(2, 1, 32, 32), rng.randn(2, 3, 32, 32)
    return Graph("patchgan", d["out"], d["inputs"], [a, b])


def _bn_groups2(rng):
    return _chain("bn_groups2", rng, (4, 8, 16, 16),
                  lambda i: _conv(_bn(_conv(i, 16, 3), LRELU), 8, 3), bn_groups=2)


def _lrelu_probe(rng):
    """conv -> lrelu(0.2) whose pre-activations are mostly negative (bias -2): the output is ~0.2 * conv, so a slope of
    0.19 moves it by ~5 % -- the graph of the non-vacuity check"""
    i, x = _inp(rng, (2, 16, 32, 32))
    c = _conv(i, 32, 3, act=LRELU)
    c.b.set_value(np.full(c.b.shape, -2.0, np.float32))
    return Graph("lrelu_probe", _conv(c, 16, 3), [i], [x])


NAMED = {
    "up_nearest_conv5": _up_nearest_conv5,
    "up_nearest_conv5_act": _up_nearest_conv5_act,
    "blconv_bn": _blconv("blconv_bn", (2, 32, 32, 32), 32, lambda c: _bn(c, LRELU)),
    "blconv_linear": _blconv("blconv_linear", (1, 32, 32, 32), 64, lambda c: c),
    "blconv_16_literal": _blconv("blconv_16_literal", (2, 32, 16, 16), 32, lambda c: _bn(c, rectify)),
    "blconv_act_lrelu": _blconv_act("blconv_act_lrelu", leaky_rectify),
    "blconv_act_tanh": _blconv_act("blconv_act_tanh", tanh),
    # the repro of defect 1: Conv2DLayer(linear) + a separate NonlinearityLayer, folded into the conv by R2
    "blconv_act_layer": _blconv("blconv_act_layer", (2, 32, 32, 32), 32, lambda c: L.NonlinearityLayer(c, leaky_rectify)),
    "blconv_c48": _blconv("blconv_c48", (2, 48, 32, 32), 32, lambda c: _bn(c)),
    "convpool_thin_relu": _convpool("convpool_thin_relu", (2, 3, 32, 32), 16, 3, rectify),
    "convpool_thin_lrelu": _convpool("convpool_thin_lrelu", (2, 1, 32, 32), 16, 5, LRELU, separate=True),
    "convpool_thin_tanh": _convpool("convpool_thin_tanh", (2, 4, 32, 32), 16, 3, tanh),
    "convpool_lp_relu": _convpool("convpool_lp_relu", (2, 16, 32, 32), 32, 3, rectify),
    "convpool_lp_lrelu": _convpool("convpool_lp_lrelu", (2, 32, 32, 32), 32, 5, LRELU, separate=True),
    "convpool_lp_tanh": _convpool("convpool_lp_tanh", (2, 16, 32, 32), 32, 3, tanh, separate=True),
    "conv_bn_act": _conv_bn_act,
    "conv_bn_act_small": _conv_bn_act_small,
    "conv_act_bn": _conv_act_bn,
    "pixel_discriminator_bn": _pixel_discriminator_bn,
    "unet_skip": _unet_skip,
    "concat_aligned": _concat("concat_aligned", (16, 16)),
    # the repro of defect 2: member slices not 8-channel aligned, their sum (32) is
    "concat_unaligned": _concat("concat_unaligned", (12, 20)),
    "concat_offset4": _concat("concat_offset4", (4, 8, 4), k_out=16),
    "concat_input_slice": _concat_input_slice,
    "stride2_odd": _stride2_odd,
    "stride2_5x5_rect": _stride2_5x5_rect,
    "small_maps": _small_maps,
    "tiny_2x2": _tiny_2x2,
    "one_filter_out": _one_filter_out,
    "one_filter_5x5": _one_filter_5x5,
    "deconv": _deconv,
    "dcgan_head": _dcgan_head,
    "dense_tail": _dense_tail,
    "instance_norm": _instance_norm,
    "dropout": _dropout,
    "avgpool2": _avgpool("avgpool2", 2),
    "avgpool4": _avgpool("avgpool4", 4),
    "patchgan": _patchgan,
    "bn_groups2": _bn_groups2,
    "lrelu_probe": _lrelu_probe,
}


# ---- generated graphs ------------------------------------------------------------------------------------------------
N_GENERATED = 30
_ACTS = (linear, rectify, LRELU, leaky_rectify, tanh, sigmoid)


def _generated(seed):
    """a chain of 2-5 blocks over the engine's vocabulary; every choice from RandomState(seed)"""
    r = np.random.RandomState(seed)
    B = int(r.choice([1, 2, 3, 4]))
    C = int(r.choice([1, 3, 8, 16, 32]))
    H = int(r.choice([8, 12, 16, 24, 32]))
    W = H if r.rand() < 0.7 else int(r.choice([8, 16, 20, 32]))
    i = L.InputLayer((None, C, H, W))
    x = i
    act = lambda: _ACTS[r.randint(len(_ACTS))]
    width = lambda: int(r.choice([1, 4, 8, 12, 16, 24, 32]))
    for _ in range(r.randint(2, 6)):
        _, C, H, W = x.output_shape
        ops = ['conv', 'conv_bn', 'conv_act_bn', 'concat', 'in', 'dropout']
        if H % 2 == 0 and W % 2 == 0 and H >= 4 and W >= 4:
            ops += ['maxpool', 'avgpool']
        if H <= 16 and W <= 16:
            ops += ['up_nearest', 'up_bilinear', 'deconv']
        if H >= 4 and W >= 4:
            ops += ['conv_s2']
        op = ops[r.randint(len(ops))]
        if op == 'conv':
            k = int(r.choice([1, 3, 5]))
            x = _conv(x, width(), k, act=act())
        elif op == 'conv_s2':
            x = _conv(x, width(), 3, stride=2, pad=1, act=act())
        elif op == 'conv_bn':
            x = _bn(_conv(x, int(r.choice([8, 16, 32])), 3), act())
        elif op == 'conv_act_bn':
            x = L.BatchNormLayer(L.NonlinearityLayer(_conv(x, int(r.choice([8, 16, 32])), 3), act()))
        elif op == 'concat':
            a = _conv(x, width(), 3, act=act())
            b = _conv(x, width(), 3, act=act())
            x = L.ConcatLayer([a, b])
            if r.rand() < 0.5:
                x = L.NonlinearityLayer(x, act())
        elif op == 'in':
            x = L.NonlinearityLayer(L.InstanceNormLayer(_conv(x, int(r.choice([8, 16])), 3)), act())
        elif op == 'dropout':
            x = L.DropoutLayer(_conv(x, width(), 3, act=act()), p=0.25)
        elif op == 'maxpool':
            x = L.MaxPool2DLayer(_conv(x, width(), 3, act=act()), 2)
        elif op == 'avgpool':
            p = 4 if (H % 4 == 0 and W % 4 == 0 and r.rand() < 0.5) else 2
            x = L.Pool2DLayer(_conv(x, width(), 3, act=act()), p, mode='average_inc_pad')
        elif op == 'up_nearest':
            x = _conv(L.Upscale2DLayer(x, 2), int(r.choice([8, 16, 32])), 5, act=act())
        elif op == 'up_bilinear':
            x = _conv(BilinearUpsample2DLayer(x, 2), int(r.choice([8, 16, 32])), 3, pad=1, act=act())
        else:
            x = L.Deconv2DLayer(x, width(), 2, stride=2, nonlinearity=act())
    if not isinstance(x, (L.Conv2DLayer, L.TransposedConv2DLayer)):
        x = _conv(x, int(r.choice([1, 4, 8])), 3)
    feed = r.rand(B, *i.output_shape[1:])
    return Graph("gen%02d" % (seed - 1000), x, [i], [feed])


GENERATED = ["gen%02d" % k for k in range(N_GENERATED)]
NAMES = list(NAMED) + GENERATED


def graph(name):
    """build graph ``name`` afresh: parameters from an initialiser RNG seeded by the graph's index, BatchNorm / InstanceNorm
    gamma / beta and the biases moved off their 1 / 0 defaults"""
    idx = NAMES.index(name)
    INIT.set_rng(np.random.RandomState(100 + idx))
    g = NAMED[name](np.random.RandomState(200 + idx)) if name in NAMED else _generated(1000 + int(name[3:]))
    prng = np.random.RandomState(300 + idx)
    for p in L.get_all_params(g.out, trainable=True):
        if p.name in ("gamma", "beta"):
            p.set_value((p.get_value() + 0.3 * prng.randn(*p.shape)).astype(np.float32))
        elif p.name.endswith(".b"):
            # non-zero biases: with the initialiser's zeros a conv behind a dead relu region outputs exact zeros, where the
            # oracle's leaky-relu derivative is Theano's 0.5 * (1 + a) and the kernels' is a (a measure-zero convention)
            p.set_value((p.get_value() + 0.1 * prng.randn(*p.shape)).astype(np.float32))
    return g


# ---- running one graph: device and float64 interpreter ---------------------------------------------------------------
def image_inputs(g):
    return [l for l in g.inputs if len(l.output_shape) == 4]


def plan_graph(dev, ops, g, dtype, store=None):
    """-> (plan, store, forward program, backward program, {InputLayer: input-gradient tensor}, seed array)"""
    from gan_heightmaps_amd.engine import NetPlan, ParamStore
    store = store or ParamStore(dev, L.get_all_params(g.out))
    plan = NetPlan(dev, ops, g.out, g.batch, store, name=g.name, dtype=dtype, bn_groups=g.bn_groups)
    fwd, bwd = [], []
    plan.emit_forward(fwd)
    seed = np.random.RandomState(2).randn(*plan.out.shape).astype(np.float32)
    gin = plan.emit_backward(bwd, dev.tensor(seed), input_grads=image_inputs(g))
    return plan, store, fwd, bwd, gin, seed


def run_on_device(dev, ops, g, dtype='f32'):
    """forward + backward (with the image-input gradients), then the deterministic forward: -> dict of host arrays"""
    plan, store, fwd, bwd, gin, seed = plan_graph(dev, ops, g, dtype)
    for l, x in zip(g.inputs, g.feeds):
        t = plan.input_tensor(l)
        t.set(x.reshape(t.shape))
    for e in fwd + bwd:
        e[1]()
    dev.sync()
    res = {"out": plan.out.numpy().copy(), "seed": seed,
           "keys": {id(n.layer): n.aux['key'] for n in plan.dropout_nodes},
           "grads": {id(p): store.download_grad(p) for p in L.get_all_params(g.out, trainable=True)},
           "gin": {id(l): gin[l].numpy().copy() for l in image_inputs(g)},
           "running": {id(l): (l.mean.get_value(), l.inv_std.get_value())
                       for l in L.get_all_layers(g.out) if isinstance(l, L.BatchNormLayer)}}
    det = []
    plan.emit_forward(det, deterministic=True)
    for e in det:
        e[1]()
    dev.sync()
    res["det"] = plan.out.numpy().copy()
    res["plan"], res["store"] = plan, store
    return res


def _golden():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if d not in sys.path:
        sys.path.insert(0, d)
    import symtheano
    return symtheano


def reference(g, seed, keys=None):
    """the same graph in float64 on the same fp32 inputs / parameters / output seed: output, every trainable parameter's
    gradient, the image-input gradients, and per BatchNormLayer the batch statistics its running statistics take (for
    bn_groups=2, each half normalised with its own statistics and the running statistics from the second half, as
    NetPlan does)"""
    ST = _golden()
    from oracle import tape as TP
    env = {"in%d" % k: x for k, x in enumerate(g.feeds)}
    env['__rng__'] = lambda l: (keys[id(l)], 1)          # the first forward pass of a plan runs with counter value 1
    c = ST.Ctx(env, np.float64)
    sym_in = {l: ST.placeholder("in%d" % k) for k, l in enumerate(g.inputs)}
    if g.bn_groups == 1:
        out = ST.get_output(g.out, sym_in).ev(c)
        stats = {id(l): (mu, inv) for l, mu, inv in c.bn}
    else:
        hb = g.batch // 2
        halves = []
        for h in (0, 1):
            ch = {"in%d" % k: x[h * hb:(h + 1) * hb] for k, x in enumerate(g.feeds)}
            sym_h = {l: ST.Sym(lambda c_, k=k, ch=ch: TP.leaf(np.asarray(ch["in%d" % k], c_.dtype))) for k, l in enumerate(g.inputs)}
            y = ST.get_output(g.out, sym_h)          # (kept alive: the context memoises by id of the expression)
            halves.append((sym_h, y, y.ev(c)))
        out = TP.concat([y for _, _, y in halves], 0)
        stats = {id(l): (mu, inv) for l, mu, inv in c.bn[len(c.bn) // 2:]}
    TP.backward(out, seed.astype(np.float64).reshape(out.v.shape))
    ref = {"out": out.v, "grads": {}, "gin": {}, "stats": stats}
    for p in L.get_all_params(g.out, trainable=True):
        ref["grads"][id(p)] = c.param(p).g
    for l in image_inputs(g):
        if g.bn_groups == 1:
            ref["gin"][id(l)] = sym_in[l].ev(c).g
        else:
            ref["gin"][id(l)] = np.concatenate([s[l].ev(c).g for s, _, _ in halves], 0)
    return ref


def reference_det(g):
    """the deterministic forward in float64: BatchNorm with the running statistics the parameters hold now (the device's,
    when a ParamStore is bound), dropout as identity"""
    ST = _golden()
    c = ST.Ctx({"in%d" % k: x for k, x in enumerate(g.feeds)}, np.float64)
    sym_in = {l: ST.placeholder("in%d" % k) for k, l in enumerate(g.inputs)}
    return ST.get_output(g.out, sym_in, deterministic=True).ev(c).v


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


def errors(g, res, ref, det_ref):
    """relative L2 errors of one device run: {'out', 'grad' (worst parameter), 'gin' (worst input), 'stats', 'det'} and
    the number of parameter gradients compared (those the reference does not give as exactly zero)"""
    e = {"out": rel(res["out"].reshape(ref["out"].shape), ref["out"]), "grad": 0.0, "gin": 0.0, "stats": 0.0,
         "det": rel(res["det"].reshape(det_ref.shape), det_ref), "checked": 0, "worst": None}
    for p in L.get_all_params(g.out, trainable=True):
        g_ref = ref["grads"][id(p)]
        if g_ref is None or np.linalg.norm(g_ref) < 1e-9:
            continue                 # e.g. a conv bias that feeds a BatchNorm: exactly zero
        r = rel(res["grads"][id(p)], g_ref)
        e["checked"] += 1
        if r >= e["grad"]:
            e["grad"], e["worst"] = r, (p.name, p.shape)
    for l in image_inputs(g):
        g_ref = ref["gin"][id(l)]
        assert g_ref is not None and np.linalg.norm(g_ref) > 0
        e["gin"] = max(e["gin"], rel(res["gin"][id(l)].reshape(g_ref.shape), g_ref))
    for lid, (mu, inv) in ref["stats"].items():
        rm, ri = res["running"][lid]
        mu, inv = mu.ravel(), inv.ravel()
        # Lasagne's update from (0, 1): 0.1 * batch statistics + 0.9 * old.  The mean's error is measured in units of the
        # channel's standard deviation (a mean near zero has no relative error to speak of)
        e["stats"] = max(e["stats"], rel(ri, 0.9 + 0.1 * inv),
                         np.linalg.norm((rm - 0.1 * mu) * inv) / (0.1 * np.sqrt(mu.size)))
    return e
