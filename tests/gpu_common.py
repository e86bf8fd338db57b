"""What the GPU test modules share beyond tests/canary.py: the device fixtures, the small model configurations and their
builders, the resume helpers, and the canvases and planes of the terrain tool tests.  A plain module: the test modules import
from here, never from one another."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import erosion as ER
from gan_heightmaps_amd import render as RN
from tests import erosion_ref


# ---- the device ----
@pytest.fixture(scope="module")
def dev():
    from gan_heightmaps_amd import device
    if device.device_count() == 0:
        pytest.fail("no HIP device visible")
    d = device.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ops(dev):
    from gan_heightmaps_amd.device import Ops
    return Ops(dev)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


# ---- models ----
SMALL = dict(in_shp=32, latent_dim=24,
             gen_dcgan=dict(nch=16, div=[2, 2, 4]),
             disc_dcgan=dict(nch=16, div=[4, 2, 2]),
             gen_p2p=dict(nf=4), disc_p2p=dict(nf=4, mul_factor=[1, 2]))

# the whole train step in reduced precision (tests/test_gpu_lp.py)
LP_STEP = dict(in_shp=128, latent_dim=32,
               gen_dcgan=dict(nch=64, div=[1, 2, 2, 2, 2]), disc_dcgan=dict(nch=64, div=[2, 2, 1, 1]),
               gen_p2p=dict(nf=16), disc_p2p=dict(nf=32, mul_factor=[1, 2, 4]))


def build_model(cfg, seed, dev=None, **kw):
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    from gan_heightmaps_amd import nonlinearities as NL, updates as UP
    g, d, u, p = cfg['gen_dcgan'], cfg['disc_dcgan'], cfg['gen_p2p'], cfg['disc_p2p']
    nl = {'linear': NL.linear, 'tanh': NL.tanh, 'sigmoid': NL.sigmoid}
    opt = UP.rmsprop if cfg['opt'] == 'rmsprop' else UP.adam
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
        opt=opt, opt_args={'learning_rate': UP.shared(np.float32(cfg['lr']))},
        train_mode=cfg['train_mode'], verbose=False, seed=seed, device=dev, **kw)


NETS = [('dcgan', 'gen', 'dcgan_gen'), ('dcgan', 'disc', 'dcgan_disc'), ('p2p', 'gen', 'p2p_gen'),
        ('p2p', 'disc', 'p2p_disc')]
NET_PAIRS = [(a, b) for a, b, _ in NETS]


def model_params(model):
    from gan_heightmaps_amd import layers as L
    return {(a, b): L.get_all_param_values(getattr(model, a)[b]) for a, b, _ in NETS}


def model_grads(model):
    from gan_heightmaps_amd import layers as L
    out = {}
    for a, b, k in NETS:
        st = model.engine.stores[k]
        out[(a, b)] = [st.download_grad(p) for p in L.get_all_params(getattr(model, a)[b], trainable=True)]
    return out


# ---- resumed runs (tests/test_gpu_resume.py; the EMA and PixelGAN tests resume too) ----
LR = {'sgd': 1e-2, 'momentum': 1e-2, 'nesterov_momentum': 1e-2, 'adagrad': 1e-3, 'rmsprop': 1e-3, 'adadelta': 1.0,
      'adam': 1e-3, 'adamax': 1e-3, 'amsgrad': 1e-3}
K, M = 3, 3


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
    return {'params': {n: L.get_all_param_values(getattr(m, n[0])[n[1]]) for n in NET_PAIRS},
            'state': m.engine.training_state()}


def assert_same(a, b):
    for n in NET_PAIRS:
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


def _iterators(dev):
    from gan_heightmaps_amd import data as D
    rng = np.random.RandomState(0)
    X = rng.randint(0, 256, (10, 32, 32, 1)).astype(np.uint8)         # 10 samples of batch 4: a ragged slice of 2
    Y = rng.randint(0, 256, (10, 32, 32, 3)).astype(np.uint8)
    imgen = D.ImageDataGenerator(horizontal_flip=True, vertical_flip=True, rotation_range=360, fill_mode="reflect")
    return D.Hdf5Iterator(X, Y, 4, imgen, True, False, device=dev), D.Hdf5Iterator(X, Y, 4, imgen, True, False, device=dev)


# ---- terrain tools ----
CANARY = 0xAB


class Canvas:
    """an output plane of H x W cells inside a larger buffer of canary bytes -- a row above and below, two cells to the left,
    the pitch's rest to the right -- in test_gpu_skylight.device_bake's manner"""

    def __init__(self, dev, H, W, dtype, pad=2):
        self.dev, self.H, self.W, self.dtype = dev, H, W, np.dtype(dtype)
        self.pitch, self.cell = W + pad, self.dtype.itemsize
        assert pad >= 2
        self.whole = np.full((H + 2) * self.pitch * self.cell, CANARY, np.uint8)
        self.base = dev.alloc(self.whole.nbytes)
        dev.h2d(self.base, self.whole)
        self.ptr = self.base + (self.pitch + 2) * self.cell

    def read(self):
        self.dev.d2h(self.whole, self.base, self.whole.nbytes)
        grid = self.whole.reshape(self.H + 2, self.pitch * self.cell)
        body = (slice(1, self.H + 1), slice(2 * self.cell, (2 + self.W) * self.cell))
        mask = np.ones(grid.shape, bool)
        mask[body] = False
        assert (grid[mask] == CANARY).all(), "bytes around the %s plane were written" % self.dtype
        return np.ascontiguousarray(grid[body]).view(self.dtype).reshape(self.H, self.W).copy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.dtype == b.dtype and np.array_equal(a, b)


def padded(dev, plane, dtype, src_pad, fill):
    """a source plane on the device with a pitch of W + src_pad and ``fill`` beyond its width -> (pointer, pitch)"""
    if plane is None:
        return None, 0
    plane = np.ascontiguousarray(plane, dtype)
    H, W = plane.shape
    src = np.full((H, W + src_pad), fill, dtype)
    src[:, :W] = plane
    ptr = dev.alloc(src.nbytes)
    dev.h2d(ptr, src)
    return ptr, W + src_pad


def scene_heights(m, hm):
    """a world's heightmap as a scene maps it: unit range, the mean of three channels"""
    planes = RN._unit_planes(hm, bool(m.is_a_grayscale), "heightmap")
    return planes[0] if planes.shape[0] == 1 else planes.astype(np.float64).mean(0).astype(np.float32)


# the eroded world of tests/test_gpu_erosion.py; the mesh, hydrology, viewshed and contour tests take their terrain from it too
N_WORLD = 3
ERO = ER.Erosion(iterations=N_WORLD, **erosion_ref.P_TEST)
