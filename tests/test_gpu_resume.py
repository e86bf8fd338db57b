"""Resumed training continues bit for bit on the MI355X.  Run A trains K then M steps; run B trains the same K steps,
writes Pix2Pix.save_checkpoint, and a fresh model built from a DIFFERENT init seed loads it and trains the same M steps.
Every parameter, BatchNorm statistic, optimiser slot, step counter, dropout counter and the losses of the last M steps
must be equal -- for every lasagne.updates rule, the split-fp32 and fp16 arithmetic, the one-rank RCCL exchange forms and
the pipelined input, and for Pix2Pix.train end to end on the device iterator.  The contrast: a resume through
save_model / load_model (parameters only) does not reproduce run A."""
import os

import numpy as np
import pytest

from oracle import step as ostep

pytestmark = pytest.mark.gpu

RULES = ['sgd', 'momentum', 'nesterov_momentum', 'adagrad', 'rmsprop', 'adadelta', 'adam', 'adamax', 'amsgrad']
LR = {'sgd': 1e-2, 'momentum': 1e-2, 'nesterov_momentum': 1e-2, 'adagrad': 1e-3, 'rmsprop': 1e-3, 'adadelta': 1.0,
      'adam': 1e-3, 'adamax': 1e-3, 'amsgrad': 1e-3}
SMALL = dict(in_shp=32, latent_dim=24,
             gen_dcgan=dict(nch=16, div=[2, 2, 4]),
             disc_dcgan=dict(nch=16, div=[4, 2, 2]),
             gen_p2p=dict(nf=4), disc_p2p=dict(nf=4, mul_factor=[1, 2]))
NETS = [('dcgan', 'gen'), ('dcgan', 'disc'), ('p2p', 'gen'), ('p2p', 'disc')]
K, M = 3, 3


@pytest.fixture(scope="module")
def dev():
    from gan_heightmaps_amd import device
    if device.device_count() == 0:
        pytest.fail("no HIP device visible")
    d = device.Device(0)
    yield d
    d.close()


def build(kind, seed, dev, **kw):
    """the nets of tests/test_dp_product.py::_nets (32^2), with the U-Net's dropout ON"""
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    from gan_heightmaps_amd import nonlinearities as NL, updates as UP
    cfg = ostep.default_cfg(**SMALL)
    return Pix2Pix(gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
                   gen_params_dcgan=dict(nch=16, div=[2, 2, 4]),
                   disc_params_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity=NL.linear),
                   gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
                   gen_params_p2p=dict(nf=4, act=NL.tanh, bilinear_upsample=True, dropout=True),
                   disc_params_p2p=dict(nf=4, act=NL.linear, mul_factor=[1, 2]),
                   in_shp=32, latent_dim=24, is_a_grayscale=True, is_b_grayscale=False,
                   alpha=cfg['alpha'], lsgan=cfg['lsgan'], reconstruction=cfg['reconstruction'],
                   opt=getattr(UP, kind), opt_args={'learning_rate': UP.shared(np.float32(LR[kind]))},
                   verbose=False, seed=seed, device=dev, **kw)


def batches(n, seed=300):
    cfg = ostep.default_cfg(**SMALL)
    return [ostep.synthetic_batch(4, cfg, seed=seed + 3 * i) for i in range(n)]


def steps(m, bs, feed):
    if feed == 'pipelined':
        return [list(r) for r in m.engine.train_pipelined(bs)]
    return [list(m.train_fn(*b)) for b in bs]


def snapshot(m):
    from gan_heightmaps_amd import layers as L
    return {'params': {n: L.get_all_param_values(getattr(m, n[0])[n[1]]) for n in NETS},
            'state': m.engine.training_state()}


def assert_same(a, b):
    for n in NETS:
        assert len(a['params'][n]) == len(b['params'][n])
        for x, y in zip(a['params'][n], b['params'][n]):            # weights and BatchNorm statistics
            assert np.array_equal(x, y), n
    sa, sb = a['state'], b['state']
    for k, v in sa['nets'].items():
        assert np.array_equal(v['hyper'], sb['nets'][k]['hyper']), k        # lr and t
        assert sorted(v['slots']) == sorted(sb['nets'][k]['slots'])
        for s, arr in v['slots'].items():
            assert np.array_equal(arr, sb['nets'][k]['slots'][s]), (k, s)
    assert sa['rng_counters'] == sb['rng_counters'] and sa['rng_counters']
    assert sa['loss_scale'] == sb['loss_scale']


def split_run(kind, dev, tmp_path, feed='call', mid=None, via='state', **kw):
    """-> (run A's last M losses + final snapshot, the resumed run's)"""
    bs = batches(K + M)
    a = build(kind, 7, dev, **kw)
    if mid is None:
        la = steps(a, bs, feed)
    else:
        la = steps(a, bs[:K - 1], feed) + (mid(a) or []) + steps(a, bs[K - 1:], feed)
    snap_a = snapshot(a)
    b = build(kind, 7, dev, **kw)
    steps(b, bs[:K - 1 if mid else K], feed)
    if mid is not None:
        mid(b)
        steps(b, bs[K - 1:K], feed)
    path = str(tmp_path / "k.model")
    c = build(kind, 1234, dev, **kw)
    if via == 'state':
        b.save_checkpoint(path, epoch=0)
        c.load_checkpoint(path)
    else:
        b.save_model(path)
        c.load_model(path)
    lc = steps(c, bs[K:], feed)
    return (la[-M:], snap_a), (lc, snapshot(c)), b


@pytest.mark.parametrize("kind", RULES)
def test_resume_is_bit_identical_f32(dev, tmp_path, kind):
    (la, sa), (lc, sc), _ = split_run(kind, dev, tmp_path, dtype='f32')
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)
    if kind in ('adam', 'adamax', 'amsgrad'):
        assert all(v['hyper'][1] == K + M for v in sc['state']['nets'].values())


@pytest.mark.parametrize("kind", ['rmsprop', 'adam', 'amsgrad'])
def test_resume_is_bit_identical_bf16x3(dev, tmp_path, kind):
    (la, sa), (lc, sc), _ = split_run(kind, dev, tmp_path, dtype='bf16x3')
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)


def test_resume_is_bit_identical_f16_mid_loss_scale_interval(dev, tmp_path):
    """saved with the dynamic loss scale between growth steps: a scale set by hand, clean steps counted since"""
    def mid(m):
        m.engine.set_loss_scale(1024.0)
    (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, mid=mid, dtype='f16')
    ls = b.engine.loss_scale_state()
    assert ls and all(st['scale'] == 1024.0 and st['clean_steps'] > 0 and st['skipped_steps'] == 0 for st in ls)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)
    assert sc['state']['loss_scale'] == sa['state']['loss_scale']


@pytest.mark.parametrize("mode", ['rs_ag', 'allreduce'])
def test_resume_is_bit_identical_through_the_one_rank_exchange(dev, tmp_path, mode):
    from gan_heightmaps_amd import device, dist
    cdev = device.Device(dev.index)
    comm = dist.Comm(cdev, 0, 1, channels=(2, 4))
    try:
        (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, dtype='f32', comm=comm, force_exchange=True,
                                          use_graph='recorded', exchange_mode=mode, bucket_mb=2048.0 / 2 ** 20)
        assert b.engine.exchange and b.engine.sharded == (mode == 'rs_ag')
        assert np.array_equal(np.asarray(la), np.asarray(lc))
        assert_same(sa, sc)
    finally:
        comm.close()
        cdev.close()


@pytest.mark.parametrize("prefetch", [True, False])
def test_resume_is_bit_identical_with_and_without_the_input_pipeline(dev, tmp_path, prefetch):
    (la, sa), (lc, sc), _ = split_run('amsgrad', dev, tmp_path, feed='pipelined' if prefetch else 'call',
                                      dtype='bf16x3', prefetch=prefetch)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)


def test_params_only_resume_does_not_reproduce_the_run(dev, tmp_path):
    """why the training state exists: Adam restarts its moments and t, dropout its masks"""
    (la, sa), (lc, sc), _ = split_run('adam', dev, tmp_path, via='params', dtype='f32')
    assert not np.array_equal(np.asarray(la), np.asarray(lc))
    assert any(not np.array_equal(x, y) for n in NETS for x, y in zip(sa['params'][n], sc['params'][n]))


# ---- Pix2Pix.train end to end on the device iterator ------------------------------------------------------------------
def _iterators(dev):
    from gan_heightmaps_amd import data as D
    rng = np.random.RandomState(0)
    X = rng.randint(0, 256, (10, 32, 32, 1)).astype(np.uint8)         # 10 samples of batch 4: a ragged slice of 2
    Y = rng.randint(0, 256, (10, 32, 32, 3)).astype(np.uint8)
    imgen = D.ImageDataGenerator(horizontal_flip=True, vertical_flip=True, rotation_range=360, fill_mode="reflect")
    return D.Hdf5Iterator(X, Y, 4, imgen, True, False, device=dev), D.Hdf5Iterator(X, Y, 4, imgen, True, False, device=dev)


def _rows(path):
    rows = [l.split(",") for l in open(path).read().strip().split("\n")]
    return [r[:-2] + r[-1:] for r in rows]          # (without the time column)


@pytest.mark.parametrize("prefetch", [True, False])
def test_train_resumed_from_a_state_checkpoint_continues_the_run(dev, tmp_path, prefetch):
    from gan_heightmaps_amd import layers as L
    out_a, out_b, models = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "models")
    np.random.seed(5)
    a = build('adam', 7, dev, prefetch=prefetch)
    a.train(*_iterators(dev), batch_size=4, num_epochs=2, out_dir=out_a)
    np.random.seed(5)
    b = build('adam', 7, dev, prefetch=prefetch)
    b.train(*_iterators(dev), batch_size=4, num_epochs=1, out_dir=out_b, model_dir=models, save_every=1,
            checkpoint_state=True)
    np.random.seed(99)                      # (the checkpoint brings the sampler's RNG state)
    c = build('adam', 4321, dev, prefetch=prefetch)
    c.train(*_iterators(dev), batch_size=4, num_epochs=1, out_dir=out_b, model_dir=models, save_every=1,
            checkpoint_state=True, resume=models + "/1.model")
    ra, rb = _rows(out_a + "/results.txt"), _rows(out_b + "/results.txt")
    assert len(ra) == len(rb) == 3 and rb[2][0] == "2"
    assert ra == rb
    assert os.path.exists(models + "/2.model")
    for n in NETS:
        for x, y in zip(L.get_all_param_values(getattr(a, n[0])[n[1]]), L.get_all_param_values(getattr(c, n[0])[n[1]])):
            assert np.array_equal(x, y), n
    sa, sc = a.engine.training_state(), c.engine.training_state()
    assert sa['rng_counters'] == sc['rng_counters'] and len(sa['rng_counters']) >= 3
