"""The 1x1 pixel discriminator (architectures/p2p.py pixel_discriminator), its experiment, and how the engine lowers it
-- on the host, with fake devices."""
import numpy as np
import pytest

from gan_heightmaps_amd import experiments, layers as L, updates
from gan_heightmaps_amd.architectures import p2p
from gan_heightmaps_amd.engine import NetPlan, ParamStore
from gan_heightmaps_amd.nonlinearities import leaky_rectify, linear, sigmoid, tanh
from gan_heightmaps_amd.step import GanStep
from tests.fake_device import PolicyDevice, PolicyOps


def _conv_layers(out):
    return [l for l in L.get_all_layers(out) if isinstance(l, L.Conv2DLayer)]


def test_pixel_discriminator_shapes_params_and_order():
    d = p2p.pixel_discriminator(32, True, False)
    out = d["out"]
    assert out.output_shape == (None, 1, 32, 32)
    assert [i.output_shape for i in d["inputs"]] == [(None, 1, 32, 32), (None, 3, 32, 32)]
    assert sum(int(np.prod(p.shape)) for p in L.get_all_params(out)) == 320 + 8320 + 129 == 8769
    convs = _conv_layers(out)
    assert [(c.num_filters, c.filter_size, c.stride, c.pad) for c in convs] == \
        [(64, (1, 1), (1, 1), (0, 0)), (128, (1, 1), (1, 1), (0, 0)), (1, (1, 1), (1, 1), (0, 0))]
    assert [c.W.shape for c in convs] == [(64, 4, 1, 1), (128, 64, 1, 1), (1, 128, 1, 1)]
    assert out.nonlinearity == sigmoid
    kinds = [type(l).__name__ for l in L.get_all_layers(out)]
    assert kinds == ['InputLayer', 'InputLayer', 'ConcatLayer', 'Conv2DLayer', 'NonlinearityLayer', 'Conv2DLayer',
                     'NonlinearityLayer', 'Conv2DLayer', 'NonlinearityLayer']
    assert not any(isinstance(l, L.BatchNormLayer) for l in L.get_all_layers(out))


def test_pixel_discriminator_bn_follows_the_nonlinearity():
    out = p2p.pixel_discriminator(16, True, False, nf=32, act=linear, bn=True)["out"]
    kinds = [type(l).__name__ for l in L.get_all_layers(out)][3:]
    assert kinds == ['Conv2DLayer', 'NonlinearityLayer', 'BatchNormLayer', 'Conv2DLayer', 'NonlinearityLayer',
                     'BatchNormLayer', 'Conv2DLayer', 'NonlinearityLayer']
    nl = [l for l in L.get_all_layers(out) if isinstance(l, L.NonlinearityLayer)]
    assert [l.nonlinearity for l in nl] == [leaky_rectify, leaky_rectify, linear]


def test_pixeld_experiment_kwargs_and_the_others_unchanged():
    kw = experiments.experiment_kwargs('test1_nobn_bilin_both_pixeld')
    base = experiments.experiment_kwargs('test1_nobn_bilin_both')
    assert kw['disc_fn_p2p'] is p2p.pixel_discriminator
    assert kw['disc_params_p2p'] == {'nf': 64, 'bn': False, 'act': linear, 'mul_factor': [1, 2]}
    for k in set(kw) | set(base):
        if k in ('disc_fn_p2p', 'disc_params_p2p', 'opt_args'):
            continue
        assert kw[k] == base[k], k
    for name in ('test1_nobn', 'test1_nobn_finetunep2p_bilin', 'test1_nobn_bilin_both'):
        k2 = experiments.experiment_kwargs(name)
        assert k2['disc_fn_p2p'] is p2p.discriminator
        assert k2['disc_params_p2p'] == {'nf': 64, 'bn': False, 'num_repeats': 0, 'act': linear,
                                         'mul_factor': [1, 2, 4, 8]}
    assert experiments.test1_nobn_bilin_both_pixeld.__name__ in experiments.main.__code__.co_names


def _plan(dev, d, B, dtype='f32'):
    out = d["out"]
    st = ParamStore(dev, L.get_all_params(out))
    return NetPlan(dev, dev.ops_class(dev), out, 2 * B, st, name="P", dtype=dtype), st


def _passes(plan, B):
    """the two ways the step differentiates the pix2pix discriminator (step.py): weight gradients over the [real | fake]
    batch, then the data gradient of the B input on the fake half"""
    i_b = plan.input_nodes[1].layer
    grads, d_prog, g_prog = [], [], []
    plan.emit_backward(d_prog, plan.dev.empty(plan.out.shape), wgrad=True, tag="dloss",
                       on_grads=lambda prog, ps: grads.extend(ps))
    gin = plan.emit_backward(g_prog, plan.dev.empty((B,) + plan.out.shape[1:]), nslice=(B, 2 * B), wgrad=False,
                             input_grads=[i_b], tag="gloss")
    return d_prog, g_prog, gin[i_b], grads


@pytest.mark.parametrize("dtype", ['f32', 'bf16x3'])
@pytest.mark.parametrize("act", [linear, sigmoid])
def test_pixel_discriminator_lowers_layer_by_layer(dtype, act):
    dev = PolicyDevice()
    d = p2p.pixel_discriminator(32, True, False, act=act)
    plan, st = _plan(dev, d, 4, dtype)
    convs = [n for n in plan.order if n.op == 'conv']
    # the leaky relus and the output nonlinearity are folded into the convolutions' epilogues; the concat is in place
    assert [n.op for n in plan.order] == ['input', 'input', 'concat', 'conv', 'conv', 'conv']
    assert [n.act for n in convs] == [leaky_rectify, leaky_rectify, act]
    assert [n.shape for n in convs] == [(8, 64, 32, 32), (8, 128, 32, 32), (8, 1, 32, 32)]
    assert plan.out.shape == (8, 1, 32, 32)
    fwd = []
    plan.emit_forward(fwd)
    assert [e[0] for e in fwd if e[0] != 'q_pack'] == ['conv_fwd'] * 3
    # 1x1 filters are served by the generic fp32 kernels in every mode: no low-precision weight pack, no q operands
    assert plan._lp_table is None and all(n.outq is None for n in plan.order)
    d_prog, g_prog, gx, grads = _passes(plan, 4)
    dl = [e[0] for e in d_prog]
    assert dl.count('conv_wgrad') == 3 and 'concat_bwd_copy' not in dl
    gl = [e[0] for e in g_prog]
    assert 'conv_wgrad' not in gl and gl.count('conv_dgrad') + gl.count('conv_dgrad_t') == 3
    assert gx.shape == (4, 3, 32, 32) and gx.nstride == 4 * 32 * 32
    params = L.get_all_params(d["out"])
    assert len(params) == 6 and sorted(id(p) for p in grads) == sorted(id(p) for p in params)


def test_pixel_discriminator_with_bn_lowers_its_batchnorms():
    plan, _ = _plan(PolicyDevice(), p2p.pixel_discriminator(32, True, False, act=linear, bn=True), 2)
    assert [n.op for n in plan.order].count('bn') == 2 and [n.op for n in plan.order].count('conv') == 3


def _gan_step(P, dtype='f32'):
    from gan_heightmaps_amd.architectures import dcgan
    import gan_heightmaps_amd.step as step_mod
    G = dcgan.default_generator(24, True, nch=16, div=[2, 2, 4])
    Dn = dcgan.default_discriminator(32, True, nch=16, div=[4, 2, 2], nonlinearity=linear)
    U = p2p.g_unet(32, True, False, nf=4, act=tanh, bilinear_upsample=True)
    spec = updates.rmsprop(learning_rate=updates.shared(1e-4))
    orig = step_mod.Ops
    step_mod.Ops = PolicyOps
    try:
        eng = GanStep(PolicyDevice(), G, Dn, U, P, 100, True, 'l1', spec, 'both', use_graph=False, two_streams=False,
                      dtype=dtype)
        return eng.built(4)
    finally:
        step_mod.Ops = orig


@pytest.mark.parametrize("dtype", ['f32', 'bf16x3'])
def test_gan_step_with_the_pixel_discriminator_on_fake_device(dtype):
    b = _gan_step(p2p.pixel_discriminator(32, True, False, act=linear), dtype)
    patch = _gan_step(p2p.discriminator(32, True, False, nf=4, act=linear, mul_factor=[1, 2]), dtype)
    assert [[e[0] for e in lane] for lane in b.update] == [[e[0] for e in lane] for lane in patch.update]
    # U writes its output straight into channels 1..3 of the discriminator's [A | B] pair buffer, as with the PatchGAN
    assert b.U.out.nstride == 4 * 32 * 32 and b.U.out.shape == (4, 3, 32, 32)
    assert b.U.out.ptr == b.P.input_tensor(b.P.input_nodes[1].layer).samples(4, 8).ptr
    assert b.P.out.shape == (8, 1, 32, 32)
