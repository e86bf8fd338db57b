"""The nine lasagne.updates rules on the host side (no GPU): spec signatures and defaults, the lasagne.updates alias of
as_lasagne, Pix2Pix / GanStep state allocation and update programs against the recording fake device.
The kernels themselves are checked in tests/test_gpu_optimizers.py."""
import inspect

import numpy as np
import pytest

from gan_heightmaps_amd import updates
from gan_heightmaps_amd.architectures import dcgan, p2p
from gan_heightmaps_amd.nonlinearities import linear, tanh
from tests.fake_device import FakeDevice

NETS = ['dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc']

# rule -> (lasagne's signature defaults, state buffers per parameter, advances t)
TABLE = {
    'sgd': ({'learning_rate': None}, 0, False),
    'momentum': ({'learning_rate': None, 'momentum': 0.9}, 1, False),
    'nesterov_momentum': ({'learning_rate': None, 'momentum': 0.9}, 1, False),
    'adagrad': ({'learning_rate': 1.0, 'epsilon': 1e-6}, 1, False),
    'rmsprop': ({'learning_rate': 1.0, 'rho': 0.9, 'epsilon': 1e-6}, 1, False),
    'adadelta': ({'learning_rate': 1.0, 'rho': 0.95, 'epsilon': 1e-6}, 2, False),
    'adam': ({'learning_rate': 0.001, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}, 2, True),
    'adamax': ({'learning_rate': 0.002, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}, 2, True),
    'amsgrad': ({'learning_rate': 0.001, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}, 3, True),
}
NEW = ['sgd', 'momentum', 'nesterov_momentum', 'adagrad', 'adadelta', 'adamax', 'amsgrad']


@pytest.mark.parametrize("kind", sorted(TABLE))
def test_spec_signature_and_defaults(kind):
    defaults, _, _ = TABLE[kind]
    fn = getattr(updates, kind)
    sig = inspect.signature(fn)
    assert list(sig.parameters) == list(defaults)
    for name, want in defaults.items():
        d = sig.parameters[name].default
        assert (d is inspect.Parameter.empty) if want is None else d == want, (kind, name, d)
    assert fn.__doc__ and ("lasagne.updates." + kind) in fn.__doc__
    spec = fn(learning_rate=0.5)
    assert spec.kind == kind and spec.learning_rate == 0.5
    assert spec.hp == {k: v for k, v in defaults.items() if k != 'learning_rate'}


@pytest.mark.parametrize("kind", NEW + ['rmsprop', 'adam'])
def test_shared_hyper_parameters_other_than_learning_rate_are_refused(kind):
    defaults, _, _ = TABLE[kind]
    fn = getattr(updates, kind)
    fn(learning_rate=updates.shared(1e-3))          # the learning rate may be shared
    for name in defaults:
        if name != 'learning_rate':
            with pytest.raises(NotImplementedError, match=name):
                fn(learning_rate=1e-3, **{name: updates.shared(defaults[name])})


def test_as_lasagne_exposes_all_nine_rules():
    from gan_heightmaps_amd import as_lasagne
    import sys
    saved = {k: sys.modules.get(k) for k in ("theano", "theano.tensor", "lasagne", "lasagne.layers", "lasagne.nonlinearities",
                                             "lasagne.init", "lasagne.updates", "lasagne.objectives", "lasagne.utils", "keras",
                                             "keras.preprocessing", "keras.preprocessing.image", "pix2pix", "util", "layers")}
    try:
        as_lasagne.install()
        import lasagne
        for kind in TABLE:
            assert getattr(lasagne.updates, kind) is getattr(updates, kind)
        assert lasagne.updates.nesterov_momentum(learning_rate=1e-4).kind == 'nesterov_momentum'
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _nets():
    G = dcgan.default_generator(24, True, nch=16, div=[2, 2, 4])
    Dn = dcgan.default_discriminator(32, True, nch=16, div=[4, 2, 2], nonlinearity=linear)
    U = p2p.g_unet(32, True, False, nf=4, act=tanh, bilinear_upsample=True)
    P = p2p.discriminator(32, True, False, nf=4, act=linear, mul_factor=[1, 2])
    return G, Dn, U, P


def _engine(spec):
    from gan_heightmaps_amd.step import GanStep
    G, Dn, U, P = _nets()
    return GanStep(FakeDevice(), G, Dn, U, P, 100, True, 'l1', spec, 'both', use_graph=False, two_streams=False)


def _pix2pix(kind, **kw):
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    return Pix2Pix(gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
                   gen_params_dcgan=dict(nch=16, div=[2, 2, 4]),
                   disc_params_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity=linear),
                   gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
                   gen_params_p2p=dict(nf=4, act=tanh), disc_params_p2p=dict(nf=4, act=linear, mul_factor=[1, 2]),
                   in_shp=32, latent_dim=24, is_a_grayscale=True, is_b_grayscale=False,
                   opt=getattr(updates, kind) if isinstance(kind, str) else kind,
                   opt_args={'learning_rate': updates.shared(np.float32(1e-4))},
                   verbose=False, seed=3, device=FakeDevice(), use_graph=False, two_streams=False, **kw)


@pytest.mark.parametrize("kind", sorted(TABLE))
def test_pix2pix_allocates_exactly_the_rules_state(kind):
    _, nstate, _ = TABLE[kind]
    m = _pix2pix(kind)
    eng = m.engine
    for k in NETS:
        st = eng.stores[k]
        assert len(st.opt_state) == nstate, (k, sorted(st.opt_state))
        ptrs = {t.ptr for t in st.opt_state.values()}
        assert len(ptrs) == nstate and st.w.ptr not in ptrs and st.g.ptr not in ptrs
        for t in st.opt_state.values():
            assert t.shape == (1, st.n_pad, 1, 1)
        assert eng.hyper[k].numpy().ravel().tolist() == [np.float32(1e-4), 0.0]


@pytest.mark.parametrize("kind", NEW)
def test_new_rule_update_program_and_launch_arguments(kind):
    defaults, nstate, ticks = TABLE[kind]
    hp = {k: v for k, v in defaults.items() if k != 'learning_rate'}
    eng = _engine(getattr(updates, kind)(learning_rate=updates.shared(1e-4)))
    b = eng.built(4)
    per_net = (lambda k: [kind + "_" + k, kind + "_tick_" + k]) if ticks else (lambda k: [kind + "_" + k])
    assert [[e[0] for e in lane] for lane in b.update] == [per_net('dcgan_gen') + per_net('dcgan_disc'),
                                                           per_net('p2p_gen') + per_net('p2p_disc')]
    for lane, ops in zip(b.update, eng.ops):
        ops.calls.clear()
        for e in lane:
            e[1]()
        names = [c[0] for c in ops.calls]
        assert 'rmsprop' not in names and 'adam' not in names
        upd = [c for c in ops.calls if c[0] == 'opt_update']
        assert len(upd) == 2 and names.count('adam_tick') == (2 if ticks else 0)
        for c in upd:
            rule, p, g, states, n, hy = c[1][:6]
            consts, gs = c[1][6], c[1][7]
            st = next(s for s in eng.stores.values() if s.w is p)
            assert rule == kind and g is st.g and n == st.n_train and hy is eng.hyper[[k for k in NETS if eng.stores[k] is st][0]]
            assert len(states) == nstate and all(s is t for s, t in zip(states, st.opt_state.values()))
            assert list(consts) == list(hp.values()) and gs == 1.0


@pytest.mark.parametrize("kind,entries", [
    ('rmsprop', lambda k: ['rmsprop_' + k]),
    ('adam', lambda k: ['adam_' + k, 'adam_tick_' + k]),
])
def test_rmsprop_and_adam_programs_are_unchanged(kind, entries):
    eng = _engine(getattr(updates, kind)(learning_rate=updates.shared(1e-4)))
    b = eng.built(4)
    assert [[e[0] for e in lane] for lane in b.update] == [entries('dcgan_gen') + entries('dcgan_disc'),
                                                           entries('p2p_gen') + entries('p2p_disc')]
    for lane, ops in zip(b.update, eng.ops):
        ops.calls.clear()
        for e in lane:
            e[1]()
        assert 'opt_update' not in [c[0] for c in ops.calls]
        assert sorted({c[0] for c in ops.calls}) == (['rmsprop'] if kind == 'rmsprop' else ['adam', 'adam_tick'])
    if kind == 'rmsprop':
        assert all(list(eng.stores[k].opt_state) == ['acc'] for k in NETS)
    else:
        assert all(list(eng.stores[k].opt_state) == ['m', 'v'] for k in NETS)


def test_unknown_kind_raises_instead_of_running_adam():
    with pytest.raises(ValueError, match="unknown optimiser kind 'adamw'"):
        _engine(updates.OptimizerSpec('adamw', 1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8))
    with pytest.raises(TypeError, match="nesterov_momentum"):
        _pix2pix(lambda learning_rate: updates.OptimizerSpec('adamw', learning_rate))
    with pytest.raises(TypeError, match="amsgrad"):
        _pix2pix(lambda learning_rate: {'kind': 'adam'})
