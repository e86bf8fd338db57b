"""The seven lasagne.updates rules of csrc/optim.hip (ghm_opt_update) on the MI355X: the kernels against float64
restatements of the rules (written from Lasagne's definitions, below), the fp16 loss-scale contract, whole train steps
through Pix2Pix against the oracle's float64 gradients, and the sharded (rs_ag) update path against the flat one.
The two op-level tests also hold the reference's own rules, rmsprop and adam (ghm_rmsprop / ghm_adam in
csrc/elementwise.hip, the oracle's rmsprop_step / adam_step in float64), to the same protocol and the same bounds."""
import sys

import numpy as np
import pytest

from oracle import ops as O
from oracle import step as ostep
from tests.gpu_common import dev      # noqa: F401  (dev: the module-scoped fixture)

pytestmark = pytest.mark.gpu

NEW = ['sgd', 'momentum', 'nesterov_momentum', 'adagrad', 'adadelta', 'adamax', 'amsgrad']
OLD = ['rmsprop', 'adam']          # entry points of their own: update() below is the adapter
NSTATE = {'rmsprop': 1, 'adam': 2, 'sgd': 0, 'momentum': 1, 'nesterov_momentum': 1, 'adagrad': 1, 'adadelta': 2, 'adamax': 2, 'amsgrad': 3}
TICKS = {'adamax', 'amsgrad', 'adam'}
# non-default constants at op level (a swapped h0 / h1 shows), in the launch order of include/ghm.h
CONSTS = {'rmsprop': (0.85, 1e-5), 'adam': (0.8, 0.99, 1e-7), 'sgd': (), 'momentum': (0.85,), 'nesterov_momentum': (0.85,), 'adagrad': (1e-5,), 'adadelta': (0.9, 1e-5),
          'adamax': (0.8, 0.99, 1e-7), 'amsgrad': (0.8, 0.99, 1e-7)}
HP_NAMES = {'sgd': (), 'momentum': ('momentum',), 'nesterov_momentum': ('momentum',), 'adagrad': ('epsilon',),
            'adadelta': ('rho', 'epsilon'), 'adamax': ('beta1', 'beta2', 'epsilon'), 'amsgrad': ('beta1', 'beta2', 'epsilon')}


def rule_ref(kind, p, g, s, lr, t, h):
    """one update of lasagne.updates.<kind> in float64.  p, g: arrays; s: the state arrays; t = t_prev + 1; h: constants.
    -> (p', [s'])"""
    if kind == 'sgd':
        return p - lr * g, []
    if kind == 'rmsprop':
        p2, a2 = O.rmsprop_step(p, g, s[0], lr, *h)
        return p2, [a2]
    if kind == 'adam':
        p2, m2, v2, _ = O.adam_step(p, g, s[0], s[1], t - 1, lr, *h)
        return p2, [m2, v2]
    if kind == 'momentum':
        (mu,) = h
        v = mu * s[0] - lr * g
        return p + v, [v]
    if kind == 'nesterov_momentum':
        (mu,) = h
        v = mu * s[0] - lr * g
        return p - lr * g + mu * v, [v]
    if kind == 'adagrad':
        (eps,) = h
        a = s[0] + g ** 2
        return p - lr * g / np.sqrt(a + eps), [a]
    if kind == 'adadelta':
        rho, eps = h
        a = rho * s[0] + (1 - rho) * g ** 2
        u = g * np.sqrt(s[1] + eps) / np.sqrt(a + eps)
        d = rho * s[1] + (1 - rho) * u ** 2
        return p - lr * u, [a, d]
    if kind == 'adamax':
        b1, b2, eps = h
        m = b1 * s[0] + (1 - b1) * g
        u = np.maximum(b2 * s[1], np.abs(g))
        return p - lr / (1 - b1 ** t) * m / (u + eps), [m, u]
    if kind == 'amsgrad':
        b1, b2, eps = h
        m = b1 * s[0] + (1 - b1) * g
        v = b2 * s[1] + (1 - b2) * g ** 2
        vh = np.maximum(s[2], v)
        return p - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(vh) + eps), [m, v, vh]
    raise ValueError(kind)


def f32(*xs):
    """the values the kernel is given: the constants and the learning rate travel as fp32 (ghm_opt_update's floats, hyper[]),
    so the float64 restatement starts from the same numbers (1 - fp32(0.99) is 1e-6 away from 0.01)"""
    return tuple(float(np.float32(x)) for x in xs)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


# ---- op level ---------------------------------------------------------------------------------------------------------

def update(ops, kind, p, g, states, n, hyper, h, grad_scale):
    """one launch of the rule: ghm_opt_update for the seven, the reference rules' own entry points for rmsprop and adam"""
    if kind == 'rmsprop':
        return ops.rmsprop(p, g, states[0], n, hyper, h[0], h[1], grad_scale)
    if kind == 'adam':
        return ops.adam(p, g, states[0], states[1], n, hyper, h[0], h[1], h[2], grad_scale)
    ops.opt_update(kind, p, g, states, n, hyper, h, grad_scale)


@pytest.mark.parametrize("n", [1003, 4096, 2 ** 24 + 3])
@pytest.mark.parametrize("kind", NEW + OLD)
def test_rule_against_float64_over_five_launches(dev, kind, n):
    """five launches on one buffer set, grad_scale 0.5, a new learning rate written into hyper between launches 2 and 3,
    gradients of changing magnitude (so that amsgrad's running max and adamax's infinity norm are not just the latest value)"""
    five_launches(dev, kind, n, 0.0)


def test_adam_from_a_large_step_count(dev):
    """the same protocol with hyper[1] starting at 10^5: powf(b, t) of the step size at a large t"""
    five_launches(dev, 'adam', 4099, 1e5)


def five_launches(dev, kind, n, t0):
    from gan_heightmaps_amd.device import Ops
    ops = Ops(dev)
    rng = np.random.RandomState(n % 1000 + len(kind))
    h = CONSTS[kind]
    lr0, lr1 = (1.0, 0.3) if kind == 'adadelta' else (1e-2, 3e-3)
    p0 = (rng.randn(n) * 0.1).astype(np.float32)
    pd, gd = dev.tensor(p0.reshape(1, n, 1, 1)), dev.zeros((1, n, 1, 1))
    sd = [dev.zeros((1, n, 1, 1)) for _ in range(NSTATE[kind])]
    hyper = dev.tensor(np.array([lr0, t0], np.float32))
    p, s, t, lr = p0.astype(np.float64), [np.zeros(n) for _ in sd], t0, lr0
    for it, mag in enumerate([1.0, 0.3, 2.0, 0.05, 1.0]):
        if it == 2:
            dev.sync()
            hv = hyper.numpy().ravel()
            hv[0] = lr = lr1
            hyper.set(hv)
        g = (rng.randn(n) * mag).astype(np.float32)
        gd.set(g)
        update(ops, kind, pd, gd, sd, n, hyper, h, 0.5)
        if kind in TICKS:
            ops.adam_tick(hyper)
        t += 1
        p, s = rule_ref(kind, p, 0.5 * g.astype(np.float64), s, f32(lr)[0], t, f32(*h))
    dev.sync()
    got_p = pd.numpy().ravel().astype(np.float64)
    assert rel(got_p - p0, p - p0) <= 1e-5, rel(got_p - p0, p - p0)
    tail = slice(n - 4 - n % 4, n)         # the last float4 and the ragged tail after it
    assert rel(got_p[tail] - p0[tail], (p - p0)[tail]) <= 1e-5
    for j, (a, b) in enumerate(zip(sd, s)):
        a = a.numpy().ravel()
        assert np.linalg.norm(b) > 0
        assert rel(a, b) <= 1e-6, (j, rel(a, b))
        assert rel(a[tail], b[tail]) <= 1e-6, j
    assert hyper.numpy().ravel()[1] == t0 + (5.0 if kind in TICKS else 0.0)


@pytest.mark.parametrize("kind", NEW + OLD)
def test_loss_scale_contract(dev, kind):
    """with a loss-scale state attached: the overflow flag leaves p, every state buffer and t bit-unchanged; a clean step at
    scale S equals the unscaled launch on g / S (S a power of two: both products are exact)"""
    from gan_heightmaps_amd.device import Ops
    ops = Ops(dev)
    rng = np.random.RandomState(5)
    n, S = 4099, 2.0 ** 15
    h = CONSTS[kind]

    def fresh():
        pd = dev.tensor(rng.randn(1, n, 1, 1).astype(np.float32))
        sd = [dev.tensor(np.abs(rng.randn(1, n, 1, 1)).astype(np.float32)) for _ in range(NSTATE[kind])]
        return pd, sd, dev.tensor(np.array([1e-2, 3.0], np.float32))

    def snap(pd, sd, hy):
        return [x.numpy().copy() for x in [pd] + sd + [hy]]

    g = (rng.randn(1, n, 1, 1) * S).astype(np.float32)
    gd, gd_unscaled = dev.tensor(g), dev.tensor(g / np.float32(S))
    ls = dev.tensor(np.array([S, 1.0 / S, 0, 1, 0, 0, 0, 0], np.float32))        # overflow flag set
    pd, sd, hy = fresh()
    before = snap(pd, sd, hy)
    dev.set_loss_scale_state(ls)
    try:
        update(ops, kind, pd, gd, sd, n, hy, h, 0.5)
        ops.adam_tick(hy)
        dev.sync()
        for a, b in zip(snap(pd, sd, hy), before):
            assert np.array_equal(a, b)
        ls.set(np.array([S, 1.0 / S, 0, 0, 0, 0, 0, 0], np.float32))             # clean step
        update(ops, kind, pd, gd, sd, n, hy, h, 0.5)
        if kind in TICKS:
            ops.adam_tick(hy)
        dev.sync()
    finally:
        dev.set_loss_scale_state(None)
    scaled = snap(pd, sd, hy)
    pd2, sd2, hy2 = dev.tensor(before[0]), [dev.tensor(x) for x in before[1:-1]], dev.tensor(before[-1])
    update(ops, kind, pd2, gd_unscaled, sd2, n, hy2, h, 0.5)
    if kind in TICKS:
        ops.adam_tick(hy2)
    dev.sync()
    unscaled = snap(pd2, sd2, hy2)
    assert not np.array_equal(scaled[0], before[0])
    for a, b in zip(scaled, unscaled):
        assert np.array_equal(a, b)


# ---- step level -------------------------------------------------------------------------------------------------------

SMALL = dict(in_shp=32, latent_dim=24,
             gen_dcgan=dict(nch=16, div=[2, 2, 4]),
             disc_dcgan=dict(nch=16, div=[4, 2, 2]),
             gen_p2p=dict(nf=4), disc_p2p=dict(nf=4, mul_factor=[1, 2]))
# learning rate of step 0 and the one set_value() puts in before step 1
STEP_LR = {'sgd': (1e-2, 5e-3), 'momentum': (1e-2, 5e-3), 'nesterov_momentum': (1e-2, 5e-3), 'adagrad': (1e-3, 5e-4),
           'adadelta': (1.0, 0.5), 'adamax': (1e-3, 5e-4), 'amsgrad': (1e-3, 5e-4)}
NETS = [('dcgan', 'gen', 'dcgan_gen'), ('dcgan', 'disc', 'dcgan_disc'), ('p2p', 'gen', 'p2p_gen'),
        ('p2p', 'disc', 'p2p_disc')]


def build_model(cfg, kind, lr, seed, dev, **kw):
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    from gan_heightmaps_amd import nonlinearities as NL, updates as UP
    g, d, u, p = cfg['gen_dcgan'], cfg['disc_dcgan'], cfg['gen_p2p'], cfg['disc_p2p']
    nl = {'linear': NL.linear, 'tanh': NL.tanh, 'sigmoid': NL.sigmoid}
    return Pix2Pix(
        gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
        gen_params_dcgan=dict(nch=g['nch'], h=g['h'], initial_size=g['initial_size'], div=g['div'],
                              bilinear_upsample=g['bilinear_upsample']),
        disc_params_dcgan=dict(nch=d['nch'], h=d['h'], div=d['div'], bn=d['bn'],
                               nonlinearity=nl[d['nonlinearity']], pool_mode=d['pool_mode']),
        gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
        gen_params_p2p=dict(nf=u['nf'], act=nl[u['act']], bilinear_upsample=u['bilinear_upsample']),
        disc_params_p2p=dict(nf=p['nf'], bn=p['bn'], act=nl[p['act']], mul_factor=p['mul_factor']),
        in_shp=cfg['in_shp'], latent_dim=cfg['latent_dim'],
        is_a_grayscale=cfg['is_a_grayscale'], is_b_grayscale=cfg['is_b_grayscale'],
        alpha=cfg['alpha'], lsgan=cfg['lsgan'], reconstruction=cfg['reconstruction'],
        opt=getattr(UP, kind), opt_args={'learning_rate': UP.shared(np.float32(lr))},
        train_mode=cfg['train_mode'], verbose=False, seed=seed, device=dev, **kw)


def model_params(model):
    from gan_heightmaps_amd import layers as L
    return {(a, b): L.get_all_param_values(getattr(model, a)[b]) for a, b, _ in NETS}


@pytest.mark.parametrize("kind", NEW)
@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_train_step_with_rule_against_oracle_gradients(dev, kind, dtype):
    """two recorded-issue steps through Pix2Pix (step 0 eager, step 1 recorded and run) with learning_rate.set_value()
    between them; after each, every parameter against the oracle's float64 gradients + the float64 rule, with the bounds
    tests/test_gpu_step.py::test_train_step_parity holds rmsprop / adam to"""
    from gan_heightmaps_amd import updates as UP
    cfg = ostep.default_cfg(**SMALL)
    lr0, lr1 = STEP_LR[kind]
    seed, B = 7, 4
    model = build_model(cfg, kind, lr0, seed, dev, dtype=dtype, use_graph='recorded')
    assert model.engine.opt_spec.hp == {k: v for k, v in getattr(UP, kind)(1.0).hp.items()}
    h = f32(*(model.engine.opt_spec.hp[c] for c in HP_NAMES[kind]))
    state = ostep.init_state(cfg, seed, np.float32)
    mp = model_params(model)
    for key in ostep.NET_ORDER:
        for a, b in zip(mp[key], state['params'][key[0]][key[1]]):
            assert np.array_equal(a, b)
    sp = ostep.specs(cfg)
    opt_state = {key: None for key in ostep.NET_ORDER}
    lr = lr0
    for it in range(2):
        if it == 1:
            model.lr.set_value(np.float32(lr1))
            lr = lr1
        Z, X, Y = ostep.synthetic_batch(B, cfg, seed=100 + it)
        fw = ostep.forward(state, Z, X, Y, np.float64)
        grads = ostep.gradients(fw, state, ostep.NET_ORDER)
        got = model.train_fn(Z, X, Y)
        assert rel(got, ostep.losses_of(fw)) < 1e-5
        for key in ostep.NET_ORDER:
            plist = state['params'][key[0]][key[1]]
            tr = [i for i, t in enumerate(sp[key].trainable) if t]
            if opt_state[key] is None:
                opt_state[key] = [[np.zeros(plist[i].shape) for _ in range(NSTATE[kind])] for i in tr]
            for j, i in enumerate(tr):
                p_new, opt_state[key][j] = rule_ref(kind, np.asarray(plist[i], np.float64), grads[key][j], opt_state[key][j],
                                                    f32(lr)[0], it + 1, h)
                plist[i] = p_new.astype(plist[i].dtype)
        ostep._apply_bn_running(state, fw)
        mp = model_params(model)
        for key in ostep.NET_ORDER:
            ref_p = state['params'][key[0]][key[1]]
            tr = [i for i, t in enumerate(sp[key].trainable) if t]
            zero_grad = {i for j, i in enumerate(tr) if np.linalg.norm(grads[key][j]) < 1e-10}
            keep = [i for i in range(len(ref_p)) if i not in zero_grad]
            assert rel(np.concatenate([mp[key][i].ravel() for i in keep]),
                       np.concatenate([np.asarray(ref_p[i], np.float64).ravel() for i in keep])) < 1e-5, (it, key)
            for i, (a, b) in enumerate(zip(mp[key], ref_p)):
                if i in zero_grad:
                    # conv bias feeding a BatchNorm: the true gradient is 0, fp32 noise may be normalised into steps of
                    # up to about lr by the scale-free rules (as for Adam in test_train_step_parity)
                    assert np.abs(a - b).max() <= 2 * max(lr0, lr1), (it, key, a.shape)
                else:
                    assert rel(a, b) < 1e-3 or np.abs(a - b).max() < 1e-6, (it, key, a.shape)
        for key in ostep.NET_ORDER:
            state['params'][key[0]][key[1]] = [a.copy() for a in mp[key]]
    for _, _, k in NETS:
        assert model.engine.hyper[k].numpy().ravel().tolist() == [np.float32(lr1), 2.0 if kind in TICKS else 0.0]


@pytest.mark.parametrize("issue", [False, "recorded"])
@pytest.mark.parametrize("kind", ['sgd', 'adadelta', 'amsgrad'])
def test_sharded_update_matches_flat_update(dev, kind, issue):
    """exchange_mode='rs_ag' on a world-1 communicator (force_exchange): the rule runs per shard on the communication
    stream, with its state sliced like the parameters, and reproduces the flat update bit for bit"""
    from gan_heightmaps_amd import device, dist
    cfg = ostep.default_cfg(**SMALL)
    lr = STEP_LR[kind][0]
    batches = [ostep.synthetic_batch(4, cfg, seed=40 + i) for i in range(3)]
    ref_model = build_model(cfg, kind, lr, 7, dev, dtype='f32', use_graph=issue)
    ref = [ref_model.train_fn(*b) for b in batches]
    ref_params = model_params(ref_model)
    cdev = device.Device(dev.index)
    comm = dist.Comm(cdev, 0, 1, channels=(2, 4))
    try:
        m = build_model(cfg, kind, lr, 7, dev, comm=comm, force_exchange=True, use_graph=issue, exchange_mode='rs_ag',
                        bucket_mb=2048.0 / 2 ** 20, dtype='f32')
        b = m.engine.built(4)
        assert m.engine.sharded
        after = [e[0] for e in b.exchange]
        upd = [e[0] for lane in b.update for e in lane]
        assert not any(l.startswith(kind + "_") for l in upd), upd
        nshard = sum(l.startswith(kind + "_shard_") for l in after)
        assert nshard >= 6 and nshard == sum(l.startswith("allgather_") for l in after)
        assert sum(l.startswith(kind + "_tick_") for l in after) == (4 if kind in TICKS else 0)
        got = [m.train_fn(*b_) for b_ in batches]
        assert np.array_equal(np.asarray(got), np.asarray(ref))
        p = model_params(m)
        for key in ref_params:
            for a, b_ in zip(p[key], ref_params[key]):
                assert np.array_equal(a, b_)
    finally:
        comm.close()
        cdev.close()


def test_reference_style_call_through_as_lasagne_trains(dev):
    """Pix2Pix(..., opt=lasagne.updates.nesterov_momentum, opt_args={'learning_rate': theano.shared(floatX(1e-4))}) with the
    names resolved through as_lasagne, as the reference's experiments pass them"""
    from gan_heightmaps_amd import as_lasagne
    names = ("theano", "theano.tensor", "lasagne", "lasagne.layers", "lasagne.nonlinearities", "lasagne.init",
             "lasagne.updates", "lasagne.objectives", "lasagne.utils", "keras", "keras.preprocessing",
             "keras.preprocessing.image", "pix2pix", "util", "layers")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        as_lasagne.install()
        import lasagne
        import theano
        from lasagne.utils import floatX
        from pix2pix import Pix2Pix
        from gan_heightmaps_amd.architectures import dcgan, p2p
        model = Pix2Pix(gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
                        gen_params_dcgan=dict(nch=16, div=[2, 2, 4]),
                        disc_params_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity=lasagne.nonlinearities.linear),
                        gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
                        gen_params_p2p=dict(nf=4), disc_params_p2p=dict(nf=4, mul_factor=[1, 2]),
                        in_shp=32, latent_dim=24, is_a_grayscale=True, is_b_grayscale=False,
                        opt=lasagne.updates.nesterov_momentum, opt_args={'learning_rate': theano.shared(floatX(1e-4))},
                        verbose=False, seed=3, device=dev)
        assert model.engine.opt_spec.kind == 'nesterov_momentum'
        before = model_params(model)
        cfg = ostep.default_cfg(**SMALL)
        for it in range(3):
            losses = model.train_fn(*ostep.synthetic_batch(4, cfg, seed=60 + it))
            assert np.all(np.isfinite(losses))
        after = model_params(model)
        for key in before:
            assert any(not np.array_equal(a, b) for a, b in zip(after[key], before[key])), key
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
