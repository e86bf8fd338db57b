"""The 1x1 pixel discriminator (architectures/p2p.py pixel_discriminator) on the MI355X, lowered layer by layer:
the whole train step against the float64 oracle with the oracle's PatchGAN restated as the pixel network (eager, captured
and replayed steps), the recorded step against the eager one, a bit-for-bit resume through save_checkpoint /
load_checkpoint (also through the one-rank sharded exchange), and two full-size steps of experiment
test1_nobn_bilin_both_pixeld."""
import numpy as np
import pytest

from oracle import nets as onets
from oracle import step as ostep
from oracle import tape as T
from tests.gpu_common import dev      # noqa: F401  (dev: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def pixel_spec(in_shp, is_a_grayscale, is_b_grayscale, nf=32, mul_factor=(1, 2, 4, 8), bn=False):
    assert not bn
    sp = onets.ParamSpec()
    prev = (1 if is_a_grayscale else 3) + (1 if is_b_grayscale else 3)
    for i, m in enumerate(mul_factor):
        sp.conv("pd_conv%d" % (i + 1), nf * m, prev, 1)
        prev = nf * m
    sp.conv("pd_out", 1, prev, 1)
    return sp


def pixel_fwd(P, a, b_img, act='sigmoid', mul_factor=(1, 2, 4, 8), bn=False, deterministic=False):
    """p2p.pixel_discriminator in the oracle's terms: concat, (1x1 conv -> leaky relu 0.01) per mul_factor, 1x1 conv, act"""
    assert not bn
    cur = onets._Cursor(P)
    x = T.concat([a, b_img])
    for _ in mul_factor:
        W, b = cur.take(2)
        x = T.lrelu(T.conv2d(x, W, b, 1, 0), 0.01)
    W, b = cur.take(2)
    return T.act(T.conv2d(x, W, b, 1, 0), act), cur


@pytest.fixture
def pixel_disc(monkeypatch):
    """every Pix2Pix built with p2p.discriminator gets the pixel discriminator, the oracle the same network"""
    from gan_heightmaps_amd.architectures import p2p
    monkeypatch.setattr(p2p, "discriminator", p2p.pixel_discriminator)
    monkeypatch.setattr(onets, "patchgan_spec", pixel_spec)
    monkeypatch.setattr(onets, "patchgan_fwd", pixel_fwd)


@pytest.mark.parametrize("variant", ["lsgan_linear_l1", "bce_sigmoid_l1", "p2p_only_l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_train_step_parity_with_the_pixel_discriminator(dev, pixel_disc, variant, dtype):
    """tests/test_gpu_step.py::test_train_step_parity's check with the pixel discriminator: 3 steps (eager, captured +
    launched, graph replay) of losses, gradients and updated parameters against the float64 oracle"""
    from tests.gpu_common import SMALL, build_model, model_grads, model_params, rel
    from gan_heightmaps_amd import layers as L
    over = dict(SMALL, disc_p2p=dict(nf=8, mul_factor=[1, 2]))
    if variant == "bce_sigmoid_l1":
        over.update(lsgan=False, disc_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity='sigmoid'),
                    disc_p2p=dict(nf=8, mul_factor=[1, 2], act='sigmoid'))
    elif variant == "p2p_only_l2":
        over.update(train_mode='p2p', reconstruction='l2')
    cfg = ostep.default_cfg(**over)
    model = build_model(cfg, 7, dev, dtype=dtype)
    convs = [l for l in L.get_all_layers(model.p2p['disc']) if isinstance(l, L.Conv2DLayer)]
    assert [l.filter_size for l in convs] == [(1, 1)] * 3
    state = ostep.init_state(cfg, 7, np.float32)
    mp = model_params(model)
    for key in ostep.NET_ORDER:
        for a, b in zip(mp[key], state['params'][key[0]][key[1]]):
            assert np.array_equal(a, b)
    for it in range(3):
        Z, X, Y = ostep.synthetic_batch(4, cfg, seed=100 + it)
        ref = ostep.train_step(state, Z, X, Y, dtype=np.float64)
        got = model.train_fn(Z, X, Y)
        assert rel(got, ref['losses']) < 1e-5, (it, got, ref['losses'])
        mg = model_grads(model)
        for key in ref['grads']:
            flat_g = np.concatenate([g.ravel() for g in mg[key]])
            flat_r = np.concatenate([g.ravel() for g in ref['grads'][key]])
            assert np.linalg.norm(flat_r) > 1e-3, "vacuous test: reference gradient is zero"
            assert rel(flat_g, flat_r) < 2e-4, (it, key, rel(flat_g, flat_r))
        mp = model_params(model)
        # the pixel discriminator's updated parameters (tests/test_gpu_step.py holds the other nets to theirs)
        for a, b in zip(mp[('p2p', 'disc')], state['params']['p2p']['disc']):
            assert rel(a, b) < 1e-5 or np.abs(a - b).max() < 1e-6, (it, a.shape)
        # keep the two sides from drifting apart through fp32 rounding: resync the oracle to the device
        for key in ostep.NET_ORDER:
            state['params'][key[0]][key[1]] = [a.copy() for a in mp[key]]


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_eager_recorded_and_captured_steps_are_bit_identical(dev, pixel_disc, dtype):
    from tests.gpu_common import SMALL, build_model, model_params
    cfg = ostep.default_cfg(**dict(SMALL, disc_p2p=dict(nf=8, mul_factor=[1, 2])))
    forms = {u: build_model(cfg, 11, dev, use_graph=u, dtype=dtype) for u in (False, 'recorded', True)}
    for it in range(4):
        Z, X, Y = ostep.synthetic_batch(4, cfg, seed=30 + it)
        losses = [m.train_fn(Z, X, Y) for m in forms.values()]
        assert losses[0] == losses[1] == losses[2], it
    ps = [model_params(m) for m in forms.values()]
    for k in ps[0]:
        for u, v, w in zip(ps[0][k], ps[1][k], ps[2][k]):
            assert np.array_equal(u, v) and np.array_equal(u, w)
    # two runs of the same form agree bit for bit
    again = build_model(cfg, 11, dev, use_graph=True, dtype=dtype)
    for it in range(4):
        again.train_fn(*ostep.synthetic_batch(4, cfg, seed=30 + it))
    for k, arrs in model_params(again).items():
        for u, v in zip(arrs, ps[2][k]):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_resume_is_bit_identical_with_the_pixel_discriminator(dev, tmp_path, pixel_disc, dtype):
    from tests.gpu_common import assert_same, split_run
    (la, sa), (lc, sc), _ = split_run('adam', dev, tmp_path, dtype=dtype)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)


def test_resume_is_bit_identical_through_the_one_rank_sharded_exchange(dev, tmp_path, pixel_disc):
    from gan_heightmaps_amd import device, dist
    from tests.gpu_common import assert_same, split_run
    cdev = device.Device(dev.index)
    comm = dist.Comm(cdev, 0, 1, channels=(2, 4))
    try:
        (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, dtype='f32', comm=comm, force_exchange=True,
                                          use_graph='recorded', exchange_mode='rs_ag', bucket_mb=2048.0 / 2 ** 20)
        assert b.engine.exchange and b.engine.sharded
        assert np.array_equal(np.asarray(la), np.asarray(lc))
        assert_same(sa, sc)
    finally:
        comm.close()
        cdev.close()


def test_pixeld_experiment_trains_two_full_size_steps(dev):
    from gan_heightmaps_amd import experiments
    model = experiments.make_model('test1_nobn_bilin_both_pixeld', device=dev, seed=0, verbose=False)
    it = experiments.ArrayIterator(*experiments.synthetic_arrays(8, 512, True, False), 4, True, False)
    out = []
    for _ in range(2):
        X, Y = next(it)
        Z = model.sampler(4, model.latent_dim).astype(np.float32)
        losses = np.asarray(model.train_fn(Z, X, Y), np.float64)
        assert losses.shape == (5,) and np.all(np.isfinite(losses))
        out.append(losses)
    assert not np.array_equal(out[0], out[1])
    P = model.engine.built(4).P
    assert P.out.shape == (8, 1, 512, 512) and [n.op for n in P.order].count('conv') == 3
