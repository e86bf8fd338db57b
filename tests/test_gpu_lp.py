"""bf16 / fp16 matrix-core convolutions (csrc/conv_lp.hip, BASELINE configs 4 / 5) through the C ABI, op by op.

Two bounds per case (rel-L2):
  * EXACT-GIVEN-ROUNDING <= 2e-5: against oracle/lp.py -- the float64 convolution of the operands rounded to
    bf16 / fp16 (nearest-even).  Products of two 8-bit (11-bit) mantissas are exact in fp32, so what is left is the
    fp32 accumulation order: this is the check that the kernels compute the right thing.
  * PRECISION <= 8e-3 (bf16) / 1.5e-3 (fp16): against the unrounded float64 convolution -- what rounding the operands
    costs (2^-9 / 2^-12 relative per operand, random signs).  This is the tolerance the reduced-precision step is
    specified to (north_star's 1e-3 is the bound of the fp32 path, which stays the default).
"""
import os

import numpy as np
import pytest

from gan_heightmaps_amd._lib import tuning_env

from oracle import lp as LP
from oracle import ops as O
from tests import canary
from tests.gpu_common import LP_STEP

pytestmark = pytest.mark.gpu

EXACT = 2e-5
PREC = {'bf16': 8e-3, 'f16': 1.5e-3}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


gpu = canary.fixtures()[0]


CASES = [
    # N, C, H, W, K, k, s, pad
    (2, 16, 32, 32, 128, 5, 1, 2),     # one slab, 5x5, 128-row tile
    (1, 32, 32, 64, 64, 5, 1, 2),      # 64-row tile, rectangular
    (2, 48, 32, 32, 160, 3, 1, 1),     # ragged filter tile (160 = 128 + 32), 3 slabs
    (1, 64, 64, 32, 40, 3, 1, 1),      # 40 filters on the 64-row tile (masked rows)
    (2, 32, 64, 64, 128, 3, 2, 1),     # 3x3 stride 2 -> 32x32, 128-row tile
    (1, 16, 64, 128, 64, 3, 2, 1),     # 3x3 stride 2, 64-row tile, rectangular
    (1, 128, 32, 32, 96, 3, 1, 1),     # 8 slabs (split-K when forced)
    (3, 80, 32, 32, 32, 5, 1, 2),      # 5 slabs, 32 filters
    (2, 128, 64, 64, 48, 3, 2, 1),     # stride-2 data gradient, 128-row tile (2 class rows per block)
    (1, 48, 128, 64, 32, 3, 2, 1),     # stride-2 data gradient, 64-row tile (4 class rows), rectangular
]
# narrow maps (16 / 8 columns: fragments of 2 x 16 / 4 x 8 pixels): forward and stride-1 data gradient only
NARROW = [
    (2, 64, 16, 16, 128, 3, 1, 1),
    (3, 32, 16, 16, 64, 5, 1, 2),
    (2, 64, 8, 8, 160, 3, 1, 1),
    (4, 48, 8, 8, 64, 5, 1, 2),
    (2, 32, 32, 32, 96, 3, 2, 1),      # stride 2 -> 16 x 16
    (2, 64, 16, 16, 64, 3, 2, 1),      # stride 2 -> 8 x 8
    (1, 32, 16, 48, 48, 3, 1, 1),      # 48 columns = 3 tiles of 16
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", NARROW)
def test_lp_conv_narrow_maps(gpu, case, dtype):
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = case
    x, Wt, b, dy = _tensors(case, sum(case))
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    wp = dev.tensor(D.pack_conv_w(Wt).ravel())
    xd, bd, dyd = dev.tensor(x), dev.tensor(b), dev.tensor(dy)
    assert ops.lp_supported(d, 0, dtype)
    wq = dev.alloc(ops.lp_weight_bytes(d, False))
    ops.lp_pack_weights(d, wp, wq, dtype, False)
    y_lp = LP.conv2d_fwd(x, Wt, b, s, pad, dtype)
    yd = dev.empty(y_lp.shape)
    ops.conv2d_fwd_lp(d, xd, wq, bd, yd, dtype, act='lrelu', alpha=0.01)
    assert rel(yd.numpy(), O.lrelu_fwd(y_lp, 0.01)) < EXACT, ("fwd", rel(yd.numpy(), O.lrelu_fwd(y_lp, 0.01)))
    if s == 1:
        assert ops.lp_supported(d, 1, dtype)
        dx_lp = LP.conv2d_vjp(x, Wt, dy, s, pad, dtype)[0]
        wqT = dev.alloc(ops.lp_weight_bytes(d, True))
        ops.lp_pack_weights(d, wp, wqT, dtype, True)
        dxd = dev.zeros(x.shape)
        ops.conv2d_dgrad_lp(d, dyd, wqT, dxd, dtype)
        assert rel(dxd.numpy(), dx_lp) < EXACT, ("dgrad", rel(dxd.numpy(), dx_lp))
        ops.conv2d_dgrad_lp(d, dyd, wqT, dxd, dtype, accumulate=True)
        assert rel(dxd.numpy(), 2 * dx_lp) < EXACT
    assert not ops.lp_supported(d, 2, dtype) or d.Wo % 32 == 0       # narrow weight gradients stay fp32


def _tensors(case, seed):
    N, C, H, W, K, k, s, pad = case
    rng = np.random.RandomState(seed)
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    dy = rng.randn(N, K, Ho, Wo).astype(np.float32)
    return x, Wt, b, dy


# the plan's tiles (64 filter rows; the smallest stride-2 data-gradient tile) and the larger ones kept behind tuning
# switches: 128 filter rows, the 16-row / 8-wave form, the 128 x 2 and 64 x 4 stride-2 data-gradient tiles
TILES = {"plan": {}, "wide": {"GHM_LP_BM": "128", "GHM_LP_RT16": "1", "GHM_LP_DGRAD_S2_TILE": "0"},
         "mid": {"GHM_LP_BM": "128", "GHM_LP_NO_RT16": "1", "GHM_LP_DGRAD_S2_TILE": "1"}}


@pytest.mark.parametrize("tiles", list(TILES))
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", CASES)
def test_lp_conv_forward_dgrad_wgrad(gpu, case, dtype, tiles):
    with tuning_env(**TILES[tiles]):
        _lp_conv_forward_dgrad_wgrad(gpu, case, dtype)


def _lp_conv_forward_dgrad_wgrad(gpu, case, dtype):
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = case
    x, Wt, b, dy = _tensors(case, sum(case))
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    wp = dev.tensor(D.pack_conv_w(Wt).ravel())
    xd, bd, dyd = dev.tensor(x), dev.tensor(b), dev.tensor(dy)
    # ---- forward ----
    assert ops.lp_supported(d, 0, dtype), "forward geometry should be served"
    wq = dev.alloc(ops.lp_weight_bytes(d, False))
    ops.lp_pack_weights(d, wp, wq, dtype, False)
    y_lp = LP.conv2d_fwd(x, Wt, b, s, pad, dtype)
    y_64 = O.conv2d_fwd(x.astype(np.float64), Wt.astype(np.float64), b.astype(np.float64), s, pad)
    yd = dev.empty(y_lp.shape)
    ops.conv2d_fwd_lp(d, xd, wq, bd, yd, dtype)
    got = yd.numpy()
    assert rel(got, y_lp) < EXACT, ("fwd exact", rel(got, y_lp))
    assert rel(got, y_64) < PREC[dtype], ("fwd precision", rel(got, y_64))
    ops.conv2d_fwd_lp(d, xd, wq, bd, yd, dtype, act='lrelu', alpha=0.2)
    assert rel(yd.numpy(), O.lrelu_fwd(y_lp, 0.2)) < EXACT
    ops.conv2d_fwd_lp(d, xd, wq, None, yd, dtype, act='tanh')
    assert rel(yd.numpy(), np.tanh(y_lp - b[None, :, None, None])) < EXACT
    # ---- gradients ----
    dx_lp, dW_lp, _ = LP.conv2d_vjp(x, Wt, dy, s, pad, dtype)
    dx_64, dW_64, _ = O.conv2d_vjp(x.astype(np.float64), Wt.astype(np.float64), dy.astype(np.float64), s, pad)
    # data gradient: at least 32 input channels (its output rows) and filters % 16 == 0 (its reduction slabs);
    # anything else stays on the fp32 kernels
    assert ops.lp_supported(d, 1, dtype) == (C >= 32 and K % 16 == 0)
    if ops.lp_supported(d, 1, dtype):
        wqT = dev.alloc(ops.lp_weight_bytes(d, True))
        ops.lp_pack_weights(d, wp, wqT, dtype, True)
        dxd = dev.zeros(x.shape)
        ops.conv2d_dgrad_lp(d, dyd, wqT, dxd, dtype)
        assert rel(dxd.numpy(), dx_lp) < EXACT, ("dgrad exact", rel(dxd.numpy(), dx_lp))
        assert rel(dxd.numpy(), dx_64) < PREC[dtype]
        ops.conv2d_dgrad_lp(d, dyd, wqT, dxd, dtype, accumulate=True)      # skip-connection accumulation
        assert rel(dxd.numpy(), 2 * dx_lp) < EXACT
        dev.free(wqT)
    assert ops.lp_supported(d, 2, dtype), "weight-gradient geometry should be served"
    ws = dev.alloc(max(ops.wgrad_lp_workspace(d), 16))
    dwd = dev.zeros((1, C * k * k * K, 1, 1))
    ops.conv2d_wgrad_lp(d, xd, dyd, dwd, ws, dtype)
    gw = D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k)
    assert rel(gw, dW_lp) < EXACT, ("wgrad exact", rel(gw, dW_lp))
    assert rel(gw, dW_64) < PREC[dtype]
    ops.conv2d_wgrad_lp(d, xd, dyd, dwd, ws, dtype, accumulate=True)
    assert rel(D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k), 2 * dW_lp) < EXACT
    for p in (wq, ws):
        dev.free(p)


def test_lp_strided_views_and_forced_splits(gpu):
    """channel slices of wider buffers (ConcatLayer in place: explicit sample strides) and split-K on both kernels"""
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = 2, 64, 32, 32, 96, 3, 1, 1
    x, Wt, b, dy = _tensors((N, C, H, W, K, k, s, pad), 5)
    wide_x = dev.zeros((N, C + 16, H, W))
    wide_y = dev.zeros((N, K + 32, H, W))
    xv, yv = wide_x.channels(16, 16 + C), wide_y.channels(32, 32 + K)
    xv.set(x)
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad, xv.nstride, yv.nstride)
    wp = dev.tensor(D.pack_conv_w(Wt).ravel())
    wq = dev.alloc(ops.lp_weight_bytes(d, False))
    ops.lp_pack_weights(d, wp, wq, 'bf16', False)
    y_lp = LP.conv2d_fwd(x, Wt, b, s, pad, 'bf16')
    for env in ({}, {"GHM_LP_SPLITS": "4"}):
        with tuning_env(**env):
            dev.memset_zero(wide_y.ptr, 4 * wide_y.size)
            ops.conv2d_fwd_lp(d, xv, wq, dev.tensor(b), yv, 'bf16')
        full = wide_y.numpy()
        assert rel(full[:, 32:], y_lp) < EXACT and not full[:, :32].any()
    yv.set(dy)
    dW_lp = LP.conv2d_vjp(x, Wt, dy, s, pad, 'bf16')[1]
    for env in ({"GHM_LP_WGRAD_SPLITS": "1"}, {"GHM_LP_WGRAD_SPLITS": "7"}, {"GHM_LP_WGRAD_SEG1": "1"}):
        with tuning_env(**env):
            ws = dev.alloc(max(ops.wgrad_lp_workspace(d), 16))
            dwd = dev.zeros((1, C * k * k * K, 1, 1))
            ops.conv2d_wgrad_lp(d, xv, yv, dwd, ws, 'bf16')
        assert rel(D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k), dW_lp) < EXACT, env


def test_lp_unsupported_geometries_are_refused(gpu):
    """the low-precision entry points never fall back silently: geometries they do not serve are refused and the
    caller keeps them on the fp32 kernels"""
    dev, ops, D = gpu
    from gan_heightmaps_amd._lib import GhmError
    for case in [(2, 1, 32, 32, 64, 5, 1, 2),      # 1 input channel (thin layer)
                 (2, 24, 32, 32, 64, 3, 1, 1),     # channels % 16 != 0
                 (2, 32, 12, 12, 64, 3, 1, 1),     # 12-wide map (neither a 8 / 16 / 32-column tile nor a small map)
                 (2, 32, 32, 32, 64, 1, 1, 0)]:    # 1x1 filter on a large map
        N, C, H, W, K, k, s, pad = case
        d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
        assert not ops.lp_supported(d, 0, 'bf16')
        with pytest.raises(GhmError):
            ops.conv2d_fwd_lp(d, dev.zeros((N, C, H, W)), dev.zeros((1, 64, 1, 1)), None, dev.zeros((N, K, d.Ho, d.Wo)), 'bf16')
    d = D.conv_desc(2, 32, 32, 32, 64, 3, 3, 1, 1)
    assert ops.lp_supported(d, 0, 'bf16') and not ops.lp_supported(d, 0, 'f32')


# ---- the whole train step in reduced precision ---------------------------------------------------------------------
# Bounds (rel-L2 against the float64 oracle of the same step), ~2x what the MI355X measures (printed by the test):
#   losses, and the gradients of the BatchNorm-free discriminators: the plain accumulation of operand rounding;
#   generators: every convolution is followed by a batch-4 BatchNorm whose backward removes the per-channel mean and
#   the xhat component of the incoming gradient -- at initialisation that is most of it (LSGAN's d loss / d image is
#   nearly the same functional at every pixel), so the relative noise of what remains is amplified (the fp32 path shows
#   the same amplification of ITS rounding: 1e-7 -> 1e-4, tests/test_gpu_step.py).  Bounded by the cosine to the exact
#   gradient and by the fp16 run of the same kernels landing ~8x closer (a defect would not scale with the mantissa).
STEP_TOL = {'bf16': dict(loss=1.5e-2, disc=6e-2, gen=0.6, cos=0.85), 'f16': dict(loss=2e-3, disc=1.3e-2, gen=0.2, cos=0.99)}
# (round 4, maps below 8 columns on the matrix cores too: measured bf16 2.4e-4 / 1.9e-2 / 0.29 (cosine 0.956), fp16 1.0e-5 / 6.2e-3 /
# 9.9e-2 (cosine 0.995); the generator figure moves by +-30 % with WHICH layers round -- the batch-4 BatchNorm chains again)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_reduced_precision_train_step(gpu, dtype):
    """Pix2Pix(dtype='bf16' | 'f16'): the joint train step with every served convolution on the low-precision matrix
    cores (fp32 master weights, BatchNorm, losses, RMSprop; fp16 with loss scale 2^15) against the float64 oracle of
    the SAME step, at a size where the 5x5 / 3x3 stride-1, the 3x3 stride-2 (forward, data and weight gradient) and
    the collapsed up-sample convolutions all take the low-precision kernels."""
    from oracle import step as ostep
    from tests.gpu_common import build_model, model_grads, model_params
    from gan_heightmaps_amd import layers as L
    dev, ops, D = gpu
    cfg = ostep.default_cfg(**LP_STEP)
    model = build_model(cfg, 7, dev, dtype=dtype, use_graph=False)
    f32 = build_model(cfg, 7, dev, dtype='f32', use_graph=False)
    assert model.engine.loss_scale == (32768.0 if dtype == 'f16' else 1.0)
    # the low-precision kernels really are in the program
    b = model.engine.built(4)
    kinds = {}
    for lane in b.train_compute:
        for e in lane:
            if len(e) > 2 and e[2] is not None and e[2].get("dtype") == dtype:
                kinds[(e[0], e[2]["kernel"])] = kinds.get((e[0], e[2]["kernel"]), 0) + 1
    labels = {k[0] for k in kinds}
    assert {"conv_fwd", "conv_dgrad", "conv_wgrad", "upconv_fwd", "upconv_dgrad", "upconv_wgrad"} <= labels, kinds
    assert any("dgrad_s2" in k[1] for k in kinds), kinds
    state = ostep.init_state(cfg, 7, np.float32)
    tol = STEP_TOL[dtype]
    worst = dict(loss=0.0, disc=0.0, gen=0.0, cos=1.0)
    for it in range(3):
        Z, X, Y = ostep.synthetic_batch(4, cfg, seed=200 + it)
        ref = ostep.train_step(state, Z, X, Y, dtype=np.float64)
        got = model.train_fn(Z, X, Y)
        exact = f32.train_fn(Z, X, Y)
        assert rel(exact, ref['losses']) < 1e-5                       # the fp32 path on the same inputs
        worst['loss'] = max(worst['loss'], rel(got, ref['losses']))
        mg = model_grads(model)
        for key in ref['grads']:
            flat_g = np.concatenate([g.ravel() for g in mg[key]]).astype(np.float64) / model.engine.loss_scale
            flat_r = np.concatenate([g.ravel() for g in ref['grads'][key]])
            which = 'disc' if key[1] == 'disc' else 'gen'
            worst[which] = max(worst[which], rel(flat_g, flat_r))
            worst['cos'] = min(worst['cos'], float(flat_g @ flat_r / (np.linalg.norm(flat_g) * np.linalg.norm(flat_r))))
        # both device models and the oracle continue from the fp32 model's parameters
        mp = model_params(f32)
        for key in ostep.NET_ORDER:
            state['params'][key[0]][key[1]] = [a.copy() for a in mp[key]]
        for (a_, b_), vals in mp.items():
            L.set_all_param_values(getattr(model, a_)[b_], vals)
    print("reduced-precision step %s: worst rel-L2 -- losses %.2e, discriminator gradients %.2e, generator gradients "
          "%.2e (cosine %.4f)" % (dtype, worst['loss'], worst['disc'], worst['gen'], worst['cos']))
    assert worst['loss'] < tol['loss'] and worst['disc'] < tol['disc'], worst
    assert worst['gen'] < tol['gen'] and worst['cos'] > tol['cos'], worst
    # master weights stay fp32
    assert all(v.dtype == np.float32 for vals in model_params(model).values() for v in vals)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "bf16x3"])
def test_reduced_precision_training_follows_the_fp32_trajectory(gpu, dtype):
    """Evidence that a reduced-precision run TRAINS (the single-step gradient bounds above are loose for the deep
    BatchNorm generators): 40 consecutive joint train steps at 128x128 from identical parameters on identical batches,
    once with fp32 products and once with bf16 / fp16 products.  The five loss curves must stay inside a band around
    the fp32 curves at every step, agree in their last-10-step means, and the reconstruction loss -- the term that
    dominates the U-Net's objective (alpha = 100) -- must fall by the same amount in both runs."""
    from oracle import step as ostep
    from tests.gpu_common import build_model
    dev, ops, D = gpu
    cfg = ostep.default_cfg(**LP_STEP)
    steps = 40
    curves = {}
    for dt in ('f32', dtype):
        model = build_model(cfg, 7, dev, dtype=dt)
        out = []
        for it in range(steps):
            Z, X, Y = ostep.synthetic_batch(4, cfg, seed=500 + it % 4)       # four batches, revisited: losses can fall
            out.append(model.train_fn(Z, X, Y))
        curves[dt] = np.asarray(out, np.float64)
        assert np.isfinite(curves[dt]).all()
        del model
    a, b = curves['f32'], curves[dtype]
    per_step = max(rel(b[i], a[i]) for i in range(steps))
    tail = rel(b[-10:].mean(axis=0), a[-10:].mean(axis=0))
    drop_a, drop_b = a[:4, 3].mean() - a[-4:, 3].mean(), b[:4, 3].mean() - b[-4:, 3].mean()
    print("trajectory %s vs f32 over %d steps: worst per-step rel-L2 of the loss vector %.3g, last-10 means %.3g, "
          "recon drop %.4f vs %.4f" % (dtype, steps, per_step, tail, drop_b, drop_a))
    # measured (MI355X): bf16 worst per-step 0.030 / last-10 means 0.0034; fp16 0.020 / 0.0018 -- the per-step figure
    # is dominated by how fast two GAN trajectories separate from ANY perturbation (fp16's 8x smaller rounding only
    # buys a factor 1.5), the window means by the rounding itself
    # ('bf16x3', the split-fp32 mode of csrc/conv_split.hip: fp32-accurate products, so its curves separate from the fp32
    # MFMA run's only as two fp32 runs with different summation orders do)
    band = {'bf16': (8e-2, 1e-2), 'f16': (6e-2, 6e-3), 'bf16x3': (2e-2, 3e-3)}[dtype]        # measured 9.9e-3 / 1.5e-3
    assert per_step < band[0] and tail < band[1], (per_step, tail)
    assert drop_a > 0 and abs(drop_b - drop_a) < 0.1 * drop_a, (drop_a, drop_b)


def test_fp16_overflow_skips_the_update_and_lowers_the_scale(gpu):
    """Dynamic loss scaling (include/ghm.h ghm_set_loss_scale_state): a loss scale that pushes gradient operands beyond
    the fp16 range (inf after v_cvt_pk_f16_f32 -> inf / nan in the fp32 sums) must not reach the master weights or the
    RMSprop state: the step is skipped on the device (no host round trip: the recorded step replays unchanged), the
    scale is halved, and training resumes by itself once the scale fits."""
    from oracle import step as ostep
    from tests.gpu_common import build_model, model_params, model_grads
    dev, ops, D = gpu
    cfg = ostep.default_cfg(**LP_STEP)
    model = build_model(cfg, 7, dev, dtype='f16', use_graph='recorded')
    eng = model.engine
    assert [s['scale'] for s in eng.loss_scale_state()] == [32768.0, 32768.0]
    Z, X, Y = ostep.synthetic_batch(4, cfg, seed=900)
    for _ in range(3):                                   # eager, record, replay: a healthy scale
        assert np.isfinite(model.train_fn(Z, X, Y)).all()
    st = eng.loss_scale_state()
    assert all(s['skipped_steps'] == 0 and s['clean_steps'] == 3 and s['scale'] == 32768.0 for s in st), st
    weights = lambda: {k: s.w.numpy().copy() for k, s in eng.stores.items()}      # trainable values (flat buffers)
    p0 = weights()
    acc0 = {k: s.opt_state['acc'].numpy().copy() for k, s in eng.stores.items()}
    eng.set_loss_scale(2.0 ** 40)                        # seeds ~1e12: every low-precision data gradient overflows
    losses = model.train_fn(Z, X, Y)
    assert np.isfinite(losses).all()                     # the losses themselves are not scaled
    assert not all(np.isfinite(g).all() for gs in model_grads(model).values() for g in gs)      # the overflow is real
    st = eng.loss_scale_state()
    assert all(s['skipped_steps'] == 1 and s['scale'] == 2.0 ** 39 and s['clean_steps'] == 0 for s in st), st
    p1 = weights()
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k           # no trainable value moved (BatchNorm running statistics do:
    for k, s in eng.stores.items():                      # they are forward-pass state, and the forward pass is sound)
        assert np.array_equal(acc0[k], s.opt_state['acc'].numpy())
    for _ in range(40):                                  # the scale walks down until the step fits, then training resumes
        assert np.isfinite(model.train_fn(Z, X, Y)).all()
    st = eng.loss_scale_state()
    assert all(s['clean_steps'] > 0 and 2.0 ** 10 <= s['scale'] < 2.0 ** 39 for s in st), st
    p2 = weights()
    assert all(np.isfinite(v).all() for v in p2.values())
    assert all(not np.array_equal(p0[k], p2[k]) for k in p0)
    assert all(np.isfinite(v).all() for vals in model_params(model).values() for v in vals)


# ---- q tensors: operands rounded once at their producer, channel-block-of-8 layout (include/ghm.h) -------------------
Q_CASES = [
    # N, C,  H,  W,  K,  k, s, pad
    (2, 32, 32, 64, 64, 3, 1, 1),
    (2, 64, 16, 32, 32, 5, 1, 2),
    (2, 32, 32, 64, 64, 3, 2, 1),
    (1, 48, 16, 16, 96, 3, 1, 1),       # 16-wide map: the narrow tiles
    (3, 32, 8, 8, 160, 3, 1, 1),        # 8-wide map, K not a multiple of the 128 / 64-row tile
]


# small maps (csrc/conv_small.hip: gather GEMM + finishing kernel): 16 x 16 down to 1 x 1, 3x3 / 5x5 / 2x2 filters, stride 1
# and 2 (forward and both data-gradient forms), ragged batch / filter counts, more pixels than one block (N * H * W > 128)
SMALL_CASES = [
    # N, C,  H,  W,  K,  k, s, pad
    (4, 64, 16, 16, 64, 3, 1, 1),       # U-Net decoder level (16 x 16)
    (4, 32, 32, 32, 96, 3, 2, 1),       # encoder 32 -> 16: the stride-2 data gradient walks 16 x 16 parity classes
    (4, 64, 16, 16, 48, 3, 2, 1),       # 16 -> 8, 48 filters (ragged row tile)
    (3, 48, 8, 8, 64, 3, 2, 1),         # 8 -> 4, three images
    (4, 32, 4, 4, 80, 3, 2, 1),         # 4 -> 2
    (4, 32, 2, 2, 64, 2, 1, 0),         # conv9 of the U-Net: 2 x 2 -> 1 x 1, 2x2 filter, no padding
    (4, 32, 4, 4, 64, 3, 1, 1),         # 4 x 4 decoder level
    (2, 16, 4, 4, 32, 5, 1, 2),         # the DCGAN generator's first 5x5 convolution
    (8, 32, 8, 8, 64, 5, 1, 2),         # discriminator tail, batch 8
    (8, 16, 16, 16, 32, 5, 1, 2),       # 2048 pixels per channel
    (1, 16, 8, 8, 16, 3, 1, 1),         # one image, 16 filters
]


@pytest.mark.parametrize("splits", [None, "1", "3"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", SMALL_CASES)
def test_small_map_products(gpu, case, dtype, splits):
    """forward product and data gradient of the small-map path against oracle/lp.py (exact given the rounding), q operand in,
    fp32 + q out (q == round(fp32) bit for bit, written into a channel slice of a wider buffer), accumulate, fp32-operand
    entry point = pack + the same kernels, forced split counts (the partial slices are summed in a fixed order: the result
    is a pure function of the split count)"""
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = case
    env = {"GHM_SM_MAXM": "4096"}          # (every case on the small-map kernels, whatever the plan's own size rule says)
    if splits is not None:
        env["GHM_SM_SPLITS"] = splits
    with tuning_env(**env):
        rng = np.random.RandomState(11)
        x = rng.randn(N, C, H, W).astype(np.float32)
        Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
        b = rng.randn(K).astype(np.float32)
        d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
        dy = rng.randn(N, K, d.Ho, d.Wo).astype(np.float32)
        R = LP.ROUND[dtype]
        assert ops.lp_supported(d, 0, dtype) and ops.lp_supported(d, 1, dtype)
        assert ops.lp_q_direct(d, 0, dtype) and ops.lp_q_direct(d, 1, dtype)
        xd, bd, dyd = dev.tensor(x), dev.tensor(b), dev.tensor(dy)
        xq = D.QTensor.empty(dev, x.shape, dtype)
        ops.q_pack(xd, xq)
        wp = dev.tensor(D.pack_conv_w(Wt).ravel())
        wq, wqT = dev.alloc(ops.lp_weight_bytes(d, False)), dev.alloc(ops.lp_weight_bytes(d, True))
        ops.lp_pack_weights(d, wp, wq, dtype, False)
        ops.lp_pack_weights(d, wp, wqT, dtype, True)
        y32, y32b = dev.empty((N, K, d.Ho, d.Wo)), dev.empty((N, K, d.Ho, d.Wo))
        yq_wide = D.QTensor.empty(dev, (N, K + 8, d.Ho, d.Wo), dtype)
        dev.memset_zero(yq_wide.ptr, yq_wide.nbytes)
        yq = yq_wide.channels(8, 8 + K)
        ops.conv2d_fwd_lp_q(d, xq, wq, bd, y32, yq, dtype, act='lrelu', alpha=0.2)
        ops.conv2d_fwd_lp(d, xd, wq, bd, y32b, dtype, act='lrelu', alpha=0.2)
        y_ref = LP.conv2d_fwd(x, Wt, b, s, pad, dtype)
        y_ref = np.where(y_ref > 0, y_ref, 0.2 * y_ref)
        assert rel(y32.numpy(), y_ref) < EXACT, rel(y32.numpy(), y_ref)
        assert np.array_equal(y32.numpy(), y32b.numpy())
        assert np.array_equal(yq.numpy(), R(y32.numpy()))
        assert not yq_wide.numpy()[:, :8].any()
        yq2 = D.QTensor.empty(dev, (N, K, d.Ho, d.Wo), dtype)
        ops.conv2d_fwd_lp_q(d, xq, wq, bd, None, yq2, dtype, act='lrelu', alpha=0.2)          # q output alone
        assert np.array_equal(yq2.numpy(), yq.numpy())
        ops.conv2d_fwd_lp_q(d, xq, wq, None, y32, None, dtype, accumulate=True)              # y += conv (no bias, linear)
        assert rel(y32.numpy(), y_ref + LP.conv2d_fwd(x, Wt, 0 * b, s, pad, dtype)) < EXACT
        # data gradient
        dyq = D.QTensor.empty(dev, dy.shape, dtype)
        ops.q_pack(dyd, dyq)
        dx32 = dev.empty(x.shape)
        dxq = D.QTensor.empty(dev, x.shape, dtype) if C % 8 == 0 else None
        ops.conv2d_dgrad_lp_q(d, dyq, wqT, dx32, dxq, dtype)
        dx_ref = LP.conv2d_vjp(x, Wt, dy, s, pad, dtype)[0]
        assert rel(dx32.numpy(), dx_ref) < EXACT, rel(dx32.numpy(), dx_ref)
        assert np.array_equal(dxq.numpy(), R(dx32.numpy()))
        ops.conv2d_dgrad_lp_q(d, dyq, wqT, dx32, dxq, dtype, accumulate=True)
        assert rel(dx32.numpy(), 2 * dx_ref) < EXACT
        assert np.array_equal(dxq.numpy(), R(dx32.numpy()))
        dx32b = dev.empty(x.shape)
        ops.conv2d_dgrad_lp(d, dyd, wqT, dx32b, dtype)
        assert rel(dx32b.numpy(), dx_ref) < EXACT


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [SMALL_CASES[i] for i in (2, 3, 4, 5, 6, 7, 10)] + [(4, 256, 16, 16, 64, 3, 1, 1), (4, 512, 32, 32, 32, 3, 2, 1)])
def test_small_map_convolution_with_the_batchnorm_in_its_finishing_kernel(gpu, case, dtype):
    """ghm_conv2d_bn_fwd_lp_q: Conv2DLayer -> BatchNormLayer -> nonlinearity (every BatchNorm-fed layer of
    architectures/p2p.py:169-240, dcgan.py:22-24) as one product on the small maps: conv_out = conv + bias (exact given the
    rounding), batch statistics (biased variance, eps 1e-4, running mean / inv_std blended with alpha 0.1),
    y = lrelu(bn(conv_out)) in fp32 and as a q tensor (== round(y) bit for bit), equal to the unfused launches"""
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = case          # (the last two: 16 x 16 maps, lp_conv_kernel in split-K form + the same finishing kernel)
    rng = np.random.RandomState(5)
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    gamma, beta = (1 + 0.2 * rng.randn(K)).astype(np.float32), (0.3 * rng.randn(K)).astype(np.float32)
    rm0, ri0 = rng.randn(K).astype(np.float32), (1 + 0.1 * rng.rand(K)).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    assert ops.conv_bn_fused_supported(d, dtype)
    R = LP.ROUND[dtype]
    xq = D.QTensor.empty(dev, x.shape, dtype)
    ops.q_pack(dev.tensor(x), xq)
    wq = dev.alloc(ops.lp_weight_bytes(d, False))
    ops.lp_pack_weights(d, dev.tensor(D.pack_conv_w(Wt).ravel()), wq, dtype, False)
    shp = (N, K, d.Ho, d.Wo)
    co, y32 = dev.empty(shp), dev.empty(shp)
    yq = D.QTensor.empty(dev, shp, dtype)
    mean, inv = dev.empty((1, K, 1, 1)), dev.empty((1, K, 1, 1))
    rm, ri = dev.tensor(rm0), dev.tensor(ri0)
    ops.conv2d_bn_fwd_lp_q(d, xq, wq, dev.tensor(b), co, y32, yq, dev.tensor(gamma), dev.tensor(beta), mean, inv, rm, ri,
                           1e-4, 0.1, dtype, act='lrelu', alpha=0.01)
    c_ref = LP.conv2d_fwd(x, Wt, b, s, pad, dtype)
    assert rel(co.numpy(), c_ref) < EXACT
    # the BatchNorm of the kernel's own fp32 conv output, in float64
    c32 = co.numpy().astype(np.float64)
    yb, mu, iv = O.bn_train_fwd(c32, beta.astype(np.float64), gamma.astype(np.float64))
    y_ref = O.lrelu_fwd(yb, 0.01)
    assert rel(mean.numpy().ravel(), mu.ravel()) < 1e-6 and rel(inv.numpy().ravel(), iv.ravel()) < 1e-6
    assert rel(y32.numpy(), y_ref) < 1e-5, rel(y32.numpy(), y_ref)
    assert np.array_equal(yq.numpy(), R(y32.numpy()))
    nm, ni = O.bn_running_update(rm0.astype(np.float64), ri0.astype(np.float64), mu.ravel(), iv.ravel())
    assert rel(rm.numpy().ravel(), nm) < 1e-6 and rel(ri.numpy().ravel(), ni) < 1e-6
    # the unfused launches (product, then the one-launch BatchNorm) land on the same values
    co2, y2 = dev.empty(shp), dev.empty(shp)
    ops.conv2d_fwd_lp_q(d, xq, wq, dev.tensor(b), co2, None, dtype)
    assert np.array_equal(co2.numpy(), co.numpy())
    m2, i2 = dev.empty((1, K, 1, 1)), dev.empty((1, K, 1, 1))
    ops.bn_forward(co2, y2, m2, i2, dev.tensor(gamma), dev.tensor(beta), dev.alloc(ops.bn_workspace(K)), None, None, 1e-4, 0.1,
                   'lrelu', 0.01)
    assert rel(y32.numpy(), y2.numpy()) < 1e-6
    # q output alone
    yq2 = D.QTensor.empty(dev, shp, dtype)
    ops.conv2d_bn_fwd_lp_q(d, xq, wq, dev.tensor(b), co, None, yq2, dev.tensor(gamma), dev.tensor(beta), mean, inv, None, None,
                           1e-4, 0.1, dtype, act='lrelu', alpha=0.01)
    assert np.array_equal(yq2.numpy(), yq.numpy())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", Q_CASES)
def test_q_tensor_products(gpu, case, dtype):
    """ghm_q_pack / ghm_q_unpack round-trip the layout; the *_q products on a q operand equal the definition on the
    rounded operand (what the fp32-input entry points compute); their q OUTPUT is exactly round(fp32 output), written
    into a channel slice of a wider q buffer without touching its neighbours; with the fp32 output omitted the q
    output is unchanged; accumulate and the fused activation go through both outputs."""
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad = case
    rng = np.random.RandomState(7)
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    dy = rng.randn(N, K, d.Ho, d.Wo).astype(np.float32)
    R = LP.ROUND[dtype]
    # layout round trip through a channel slice of a wider q buffer
    wide_q = D.QTensor.empty(dev, (N, C + 16, H, W), dtype)
    dev.memset_zero(wide_q.ptr, wide_q.nbytes)
    xq = wide_q.channels(8, 8 + C)
    xd = dev.tensor(x)
    ops.q_pack(xd, xq)
    assert np.array_equal(xq.numpy(), R(x))
    full = wide_q.numpy()
    assert not full[:, :8].any() and not full[:, 8 + C:].any()
    back = dev.zeros(x.shape)
    ops.q_unpack(xq, back)
    assert np.array_equal(back.numpy(), R(x))
    # forward: q operand -> fp32 + q outputs
    wp = dev.tensor(D.pack_conv_w(Wt).ravel())
    wq, wqT = dev.alloc(ops.lp_weight_bytes(d, False)), dev.alloc(ops.lp_weight_bytes(d, True))
    ops.lp_pack_weights(d, wp, wq, dtype, False)
    ops.lp_pack_weights(d, wp, wqT, dtype, True)
    bd = dev.tensor(b)
    y32, y32b = dev.empty((N, K, d.Ho, d.Wo)), dev.empty((N, K, d.Ho, d.Wo))
    yq_wide = D.QTensor.empty(dev, (N, K + 8, d.Ho, d.Wo), dtype)
    dev.memset_zero(yq_wide.ptr, yq_wide.nbytes)
    yq = yq_wide.channels(8, 8 + K)
    ops.conv2d_fwd_lp_q(d, xq, wq, bd, y32, yq, dtype, act='lrelu', alpha=0.2)
    ops.conv2d_fwd_lp(d, xd, wq, bd, y32b, dtype, act='lrelu', alpha=0.2)
    y_ref = LP.conv2d_fwd(x, Wt, b, s, pad, dtype)
    y_ref = np.where(y_ref > 0, y_ref, 0.2 * y_ref)
    assert rel(y32.numpy(), y_ref) < EXACT
    assert np.array_equal(y32.numpy(), y32b.numpy())              # the fp32-input entry point = pack + the same kernel
    assert np.array_equal(yq.numpy(), R(y32.numpy()))
    assert not yq_wide.numpy()[:, :8].any()
    if ops.lp_q_direct(d, 0, dtype):                              # q output alone (no fp32 tensor written)
        yq2 = D.QTensor.empty(dev, (N, K, d.Ho, d.Wo), dtype)
        ops.conv2d_fwd_lp_q(d, xq, wq, bd, None, yq2, dtype, act='lrelu', alpha=0.2)
        assert np.array_equal(yq2.numpy(), yq.numpy())
    # data gradient: dy as a q tensor -> dx fp32 + q, then accumulate
    dyd = dev.tensor(dy)
    dyq = D.QTensor.empty(dev, dy.shape, dtype)
    ops.q_pack(dyd, dyq)
    dx32 = dev.empty(x.shape)
    dxq = D.QTensor.empty(dev, x.shape, dtype)
    ops.conv2d_dgrad_lp_q(d, dyq, wqT, dx32, dxq, dtype)
    dx_ref = LP.conv2d_vjp(x, Wt, dy, s, pad, dtype)[0]
    assert rel(dx32.numpy(), dx_ref) < EXACT
    assert np.array_equal(dxq.numpy(), R(dx32.numpy()))
    ops.conv2d_dgrad_lp_q(d, dyq, wqT, dx32, dxq, dtype, accumulate=True)
    assert rel(dx32.numpy(), 2 * dx_ref) < EXACT
    assert np.array_equal(dxq.numpy(), R(dx32.numpy()))
    if ops.lp_q_direct(d, 1, dtype):
        dxq2 = D.QTensor.empty(dev, x.shape, dtype)
        ops.conv2d_dgrad_lp_q(d, dyq, wqT, None, dxq2, dtype)
        assert rel(dxq2.numpy(), R(dx_ref.astype(np.float32))) < 2.0 ** -7


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_q_pooled_convolution_and_fused_activation_backward(gpu, dtype):
    """conv + LeakyReLU + 2x2 max-pool from a q operand: pooled fp32, pooled q and the arg-max mask equal the fp32-input
    form; the stride-2 data gradient with the producer's LeakyReLU backward in its epilogue writes dx as fp32 and q."""
    dev, ops, D = gpu
    R = LP.ROUND[dtype]
    rng = np.random.RandomState(3)
    N, C, H, W, K, k = 2, 32, 32, 64, 64, 5
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, 1, 2)
    assert ops.conv_pool_supported(d, 'lrelu', dtype) == 2
    xd, bd = dev.tensor(x), dev.tensor(b)
    wq = dev.alloc(ops.lp_weight_bytes(d, False))
    ops.lp_pack_weights(d, dev.tensor(D.pack_conv_w(Wt).ravel()), wq, dtype, False)
    xq = D.QTensor.empty(dev, x.shape, dtype)
    ops.q_pack(xd, xq)
    pa, pb = dev.empty((N, K, H // 2, W // 2)), dev.empty((N, K, H // 2, W // 2))
    ma, mb = dev.alloc(N * K * H * W // 4), dev.alloc(N * K * H * W // 4)
    pq = D.QTensor.empty(dev, (N, K, H // 2, W // 2), dtype)
    ops.conv2d_fwd_pool(d, xd, wq, bd, pa, ma, 'lrelu', 0.2, dtype)
    ops.conv2d_fwd_pool_lp_q(d, xq, wq, bd, pb, pq, mb, 'lrelu', 0.2, dtype)
    assert np.array_equal(pa.numpy(), pb.numpy())
    assert np.array_equal(pq.numpy(), R(pa.numpy()))
    m1, m2 = np.empty(N * K * H * W // 4, np.uint8), np.empty(N * K * H * W // 4, np.uint8)
    dev.d2h(m1, ma, m1.nbytes)
    dev.d2h(m2, mb, m2.nbytes)
    assert np.array_equal(m1, m2)
    pq2 = D.QTensor.empty(dev, (N, K, H // 2, W // 2), dtype)
    ops.conv2d_fwd_pool_lp_q(d, xq, wq, bd, None, pq2, mb, 'lrelu', 0.2, dtype)      # q output alone
    assert np.array_equal(pq2.numpy(), pq.numpy())
    # stride-2 data gradient * lrelu'(y) with a q gradient operand
    N, C, H, W, K = 8, 64, 64, 128, 64
    d2 = D.conv_desc(N, C, H, W, K, 3, 3, 2, 1)
    if ops.dgrad_dact_supported(d2, dtype) != 3:
        pytest.skip("single-pass stride-2 data gradient not planned for this geometry")
    Wt = (rng.randn(K, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32)
    dy = rng.randn(N, K, d2.Ho, d2.Wo).astype(np.float32)
    y = rng.randn(N, C, H, W).astype(np.float32)
    wqT = dev.alloc(ops.lp_weight_bytes(d2, True))
    ops.lp_pack_weights(d2, dev.tensor(D.pack_conv_w(Wt).ravel()), wqT, dtype, True)
    dyd, yd = dev.tensor(dy), dev.tensor(y)
    dyq = D.QTensor.empty(dev, dy.shape, dtype)
    ops.q_pack(dyd, dyq)
    dxa, dxb = dev.empty(y.shape), dev.empty(y.shape)
    dxq = D.QTensor.empty(dev, y.shape, dtype)
    ops.conv2d_dgrad_dact(d2, dyd, wqT, dxa, yd, 'lrelu', 0.2, dtype)
    ops.conv2d_dgrad_dact_lp_q(d2, dyq, wqT, dxb, dxq, yd, 'lrelu', 0.2, dtype)
    assert np.array_equal(dxa.numpy(), dxb.numpy())
    assert np.array_equal(dxq.numpy(), R(dxa.numpy()))
    ref = LP.conv2d_vjp(np.zeros_like(y), Wt, dy, 2, 1, dtype)[0] * np.where(y > 0, 1.0, 0.2)
    assert rel(dxa.numpy(), ref) < EXACT


WQ_CASES = [
    # N, C,   H,  W,   K,  s, k
    (2, 64,  16, 64,  128, 1, 3),   # channel groups 2 x filter tiles 4, 64-pixel strips
    (2, 128, 12, 32,  64,  1, 3),   # 4 x 2 (K = 64), 32-pixel strips, Ho not a multiple of the split
    (1, 64,  32, 128, 128, 2, 3),   # stride 2: parity planes, two new x rows per slab
    (3, 128, 16, 64,  256, 2, 3),
    (2, 64,  8,  96,  128, 1, 3),   # Wo = 96: three 32-pixel strips
    (2, 32,  24, 64,  64,  1, 5),   # 5x5: ten waves = five filter rows x two filter tiles
    (1, 64,  16, 32,  128, 1, 5),
    (3, 128, 16, 16,  128, 1, 3),   # 16-wide maps: one 16-pixel k-step per output row
    (2, 256, 16, 48,  64,  1, 3),   # 4 x 2 tile, three 16-pixel strips
    (2, 64,  32, 32,  128, 2, 3),   # stride 2 -> 16 x 16
    (2, 64,  16, 16,  64,  1, 5),   # 5x5 on a 16-wide map
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("splits", [None, "1", "3"])
@pytest.mark.parametrize("case", WQ_CASES)
def test_q_weight_gradient(gpu, case, splits, dtype):
    """ghm_conv2d_wgrad_lp_q: both operands as q tensors, read from LDS with the transposing read (the contraction runs
    over pixels, a q unit holds 8 channels): equals the definition on the rounded operands for every tile variant,
    stride, strip width and split of the rows (forced split counts include ones that do not divide Ho); accumulate."""
    dev, ops, D = gpu
    N, C, H, W, K, s, k = case
    d = D.conv_desc(N, C, H, W, K, k, k, s, k // 2)
    assert ops.lp_wgrad_q_supported(d, dtype)
    rng = np.random.RandomState(5)
    x = rng.randn(N, C, H, W).astype(np.float32)
    dy = rng.randn(N, K, d.Ho, d.Wo).astype(np.float32)
    xq, dyq = D.QTensor.empty(dev, x.shape, dtype), D.QTensor.empty(dev, dy.shape, dtype)
    ops.q_pack(dev.tensor(x), xq)
    ops.q_pack(dev.tensor(dy), dyq)
    ref = LP.conv2d_vjp(x, np.zeros((K, C, k, k), np.float32), dy, s, k // 2, dtype)[1]
    with tuning_env(**({"GHM_LP_WGRAD_SPLITS": splits} if splits else {})):
        ws = dev.alloc(max(ops.wgrad_lp_workspace(d), 16))
        dwd = dev.zeros((1, C * k * k * K, 1, 1))
        ops.conv2d_wgrad_lp_q(d, xq, dyq, dwd, ws, dtype)
        got = D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k)
        assert rel(got, ref) < EXACT, rel(got, ref)
        ops.conv2d_wgrad_lp_q(d, xq, dyq, dwd, ws, dtype, accumulate=True)
        assert rel(D.unpack_conv_w(dwd.numpy().ravel(), K, C, k, k), 2 * ref) < EXACT


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [(8, 1, 64, 64, 64, 5, 1, 2, True), (2, 4, 256, 256, 64, 3, 2, 1, False),
                                  (2, 1, 256, 256, 64, 3, 2, 1, False), (4, 1, 128, 128, 64, 5, 1, 2, True),
                                  (2, 3, 128, 256, 64, 3, 1, 1, False)])
def test_thin_first_layer_forward_writes_its_q_copy(gpu, case, dtype):
    """ghm_conv2d_fwd_thin_q / ghm_conv2d_fwd_pool_thin_q (<= 4 input channels, fp32 operands): the fp32 result (and the
    mask of the pooled form) is bit-identical to the plain entry point's, the q copy is exactly its rounding, written into a
    channel slice of a wider q buffer without touching the neighbours."""
    dev, ops, D = gpu
    N, C, H, W, K, k, s, pad, pooled = case
    rng = np.random.RandomState(sum(case[:8]))
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, s, pad)
    assert ops.thin_fwd_q_supported(d, 'lrelu', pooled, dtype)
    R = LP.ROUND[dtype]
    wp = dev.tensor(D.pack_conv_w(Wt).ravel())
    xd, bd = dev.tensor(x), dev.tensor(b)
    Ho, Wo = (d.Ho // 2, d.Wo // 2) if pooled else (d.Ho, d.Wo)
    y1, y2 = dev.empty((N, K, Ho, Wo)), dev.empty((N, K, Ho, Wo))
    wide = D.QTensor.empty(dev, (N, K + 16, Ho, Wo), dtype)
    dev.memset_zero(wide.ptr, wide.nbytes)
    yq = wide.channels(8, 8 + K)
    if pooled:
        # (the fp32-operand kernel: what the pooled entry point runs where the matrix-core kernel of the next test refuses)
        with tuning_env(GHM_NO_THIN_LP="1"):
            m1, m2 = dev.alloc(N * K * Ho * Wo), dev.alloc(N * K * Ho * Wo)
            ops.conv2d_fwd_pool(d, xd, wp, bd, y1, m1, 'lrelu', 0.2, 'f32')
            ops.conv2d_fwd_pool_thin_q(d, xd, wp, bd, y2, m2, yq, 'lrelu', 0.2)
            a, bb = np.empty(N * K * Ho * Wo, np.uint8), np.empty(N * K * Ho * Wo, np.uint8)
            dev.d2h(a, m1, a.nbytes)
            dev.d2h(bb, m2, bb.nbytes)
            assert np.array_equal(a, bb)
            assert np.array_equal((a >> 4) & 1, (y1.numpy().ravel() > 0).astype(np.uint8))      # bit 4: sign of the pooled value
            wide3 = D.QTensor.empty(dev, (N, K, Ho, Wo), dtype)                                 # q copy and mask only
            m3 = dev.alloc(N * K * Ho * Wo)
            ops.conv2d_fwd_pool_thin_q(d, xd, wp, bd, None, m3, wide3, 'lrelu', 0.2)
            dev.d2h(bb, m3, bb.nbytes)
            assert np.array_equal(a, bb) and np.array_equal(wide3.numpy(), R(y1.numpy()))
    else:
        ops.conv2d_fwd(d, xd, wp, bd, y1, 'lrelu', 0.2)
        ops.conv2d_fwd_thin_q(d, xd, wp, bd, y2, yq, 'lrelu', 0.2)
    assert np.array_equal(y1.numpy(), y2.numpy())
    assert np.array_equal(yq.numpy(), R(y1.numpy()))
    full = wide.numpy()
    assert not full[:, :8].any() and not full[:, 8 + K:].any()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [(8, 1, 64, 64, 5, 'lrelu'), (2, 1, 128, 256, 5, 'lrelu'), (3, 1, 64, 128, 3, 'relu'),
                                  (2, 3, 32, 64, 3, 'lrelu'), (2, 2, 40, 64, 3, 'linear')])
def test_pooled_first_layer_on_the_matrix_cores(gpu, case, dtype):
    """thin_pool_lp (csrc/conv_thin_lp.hip) behind ghm_conv2d_fwd_pool_thin_q: Conv2DLayer(<= 4 -> 64) -> nonlinearity ->
    MaxPool2DLayer(2) (architectures/dcgan.py:42-47) with the taps on the bf16 / fp16 matrix cores.  The convolution is
    oracle/lp.py's conv(round(x), round(W)) + b; the q copy is exactly the rounding of the kernel's own fp32 result (also
    when the fp32 result is not written, and into a channel slice of a wider buffer); the mask marks every tie of the
    window, agrees with the oracle's arg-max wherever the window has a clear winner, and carries the sign of the pooled
    value in bit 4."""
    dev, ops, D = gpu
    N, C, H, W, k, act = case
    K, pad = 64, k // 2
    rng = np.random.RandomState(sum(case[:5]))
    x = rng.randn(N, C, H, W).astype(np.float32)
    Wt = (rng.randn(K, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    d = D.conv_desc(N, C, H, W, K, k, k, 1, pad)
    assert ops.thin_fwd_q_supported(d, act, True, dtype)
    assert ops.thin_pool_lp_served(d, act, 0.2, dtype)
    R = LP.ROUND[dtype]
    wp, xd, bd = dev.tensor(D.pack_conv_w(Wt).ravel()), dev.tensor(x), dev.tensor(b)
    Hp, Wp = H // 2, W // 2
    y = dev.empty((N, K, Hp, Wp))
    wide = D.QTensor.empty(dev, (N, K + 16, Hp, Wp), dtype)
    dev.memset_zero(wide.ptr, wide.nbytes)
    yq = wide.channels(8, 8 + K)
    m = dev.alloc(N * K * Hp * Wp)
    ops.conv2d_fwd_pool_thin_q(d, xd, wp, bd, y, m, yq, act, 0.2)
    mask = np.empty(N * K * Hp * Wp, np.uint8)
    dev.d2h(mask, m, mask.nbytes)
    mask = mask.reshape(N, K, Hp, Wp)
    ref = LP.conv2d_fwd(x, Wt, b, 1, pad, dtype)
    ref = {'lrelu': lambda v: np.where(v > 0, v, 0.2 * v), 'relu': lambda v: np.maximum(v, 0), 'linear': lambda v: v}[act](ref)
    win = ref.reshape(N, K, Hp, 2, Wp, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, K, Hp, Wp, 4)
    got = y.numpy()
    assert rel(got, win.max(-1)) < EXACT, rel(got, win.max(-1))
    assert np.array_equal(yq.numpy(), R(got))
    full = wide.numpy()
    assert not full[:, :8].any() and not full[:, 8 + K:].any()
    assert np.array_equal((mask >> 4) & 1, (got > 0).astype(np.uint8))
    assert not (mask >> 5).any() and (mask & 15).all()
    srt = np.sort(win, -1)
    clear = (srt[..., 3] - srt[..., 2]) > 1e-4 * np.abs(ref).max()
    assert clear.mean() > 0.5
    assert np.array_equal((mask & 15)[clear], (1 << win.argmax(-1))[clear].astype(np.uint8))
    if act == 'relu':                       # an all-negative window is a four-way tie at zero
        dead = (win.max(-1) == 0) & (srt[..., 3] - srt[..., 0] == 0)
        assert dead.any() and ((mask & 15)[dead] == 15).all()
    # q copy and mask only (what the engine asks for when every consumer of the pooled tensor reads q)
    only = D.QTensor.empty(dev, (N, K, Hp, Wp), dtype)
    m2 = dev.alloc(N * K * Hp * Wp)
    ops.conv2d_fwd_pool_thin_q(d, xd, wp, bd, None, m2, only, act, 0.2)
    mask2 = np.empty(N * K * Hp * Wp, np.uint8)
    dev.d2h(mask2, m2, mask2.nbytes)
    assert np.array_equal(mask2.reshape(mask.shape), mask) and np.array_equal(only.numpy(), R(got))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_elementwise_producers_with_a_q_epilogue(gpu, dtype):
    """ghm_bn_apply_q, ghm_bn_backward_q, ghm_upsample_bilinear2_fwd_q, ghm_pp_to_hi_q, ghm_maxpool2_mask_bwd_q: the fp32
    result is bit-identical to the plain entry point's, the q result is exactly its rounding (also into a channel slice
    of a wider q buffer), and with the fp32 pointer NULL the q result is unchanged."""
    dev, ops, D = gpu
    R = LP.ROUND[dtype]
    rng = np.random.RandomState(12)
    N, C, H, W = 3, 24, 10, 12

    def qbuf(shape, pad=8):
        wide = D.QTensor.empty(dev, (shape[0], shape[1] + 2 * pad, shape[2], shape[3]), dtype)
        dev.memset_zero(wide.ptr, wide.nbytes)
        return wide, wide.channels(pad, pad + shape[1])

    def check_q(wide, q, ref32, pad=8):
        assert np.array_equal(q.numpy(), R(ref32))
        full = wide.numpy()
        assert not full[:, :pad].any() and not full[:, pad + ref32.shape[1]:].any()

    # ---- BatchNorm apply / backward (statistics from ghm_bn_stats: > BN_SMALL_MAX values per channel not needed) ----
    x = rng.randn(N, C, H, W).astype(np.float32) * 2 + 0.5
    g, b = (rng.rand(C) + 0.5).astype(np.float32), rng.randn(C).astype(np.float32)
    xd, gd, bd = dev.tensor(x), dev.tensor(g), dev.tensor(b)
    mean, inv = dev.empty((1, C, 1, 1)), dev.empty((1, C, 1, 1))
    ws = dev.alloc(ops.bn_workspace(C))
    ops.bn_stats(xd, mean, inv, ws)
    y1, y2 = dev.empty(x.shape), dev.empty(x.shape)
    ops.bn_apply(xd, y1, mean, inv, gd, bd, 'lrelu', 0.2)
    wide, yq = qbuf(x.shape)
    ops.bn_apply_q(xd, y2, mean, inv, gd, bd, yq, 'lrelu', 0.2)
    assert np.array_equal(y1.numpy(), y2.numpy())
    check_q(wide, yq, y1.numpy())
    wide2, yq2 = qbuf(x.shape)
    ops.bn_apply_q(xd, None, mean, inv, gd, bd, yq2, 'lrelu', 0.2)
    assert np.array_equal(yq2.numpy(), yq.numpy())
    dout = rng.randn(N, C, H, W).astype(np.float32)
    dd = dev.tensor(dout)
    dx1, dx2 = dev.empty(x.shape), dev.empty(x.shape)
    dg1, db1, dg2, db2 = (dev.zeros((1, C, 1, 1)) for _ in range(4))
    with tuning_env(GHM_NO_BN_SMALL="1"):                       # the three-pass form: the q form's reductions
        ops.bn_backward(dd, y1, xd, dx1, mean, inv, gd, dg1, db1, ws, 'lrelu', 0.2)
    wide, dxq = qbuf(x.shape)
    ops.bn_backward_q(dd, y1, xd, dx2, mean, inv, gd, dg2, db2, ws, dxq, 'lrelu', 0.2)
    # (the apply pass is a kernel of its own: the compiler contracts its multiply-adds differently -> last-bit differences)
    assert rel(dx2.numpy(), dx1.numpy()) < 1e-6 and np.array_equal(dg1.numpy(), dg2.numpy()) and np.array_equal(db1.numpy(), db2.numpy())
    check_q(wide, dxq, dx2.numpy())
    wide2, dxq2 = qbuf(x.shape)
    ops.bn_backward_q(dd, y1, xd, None, mean, inv, gd, dg2, db2, ws, dxq2, 'lrelu', 0.2)
    assert np.array_equal(dxq2.numpy(), dxq.numpy())
    wide3, dxq3 = qbuf(x.shape)          # without y: recomputed from x (the form the step issues)
    ops.bn_backward_q(dd, None, xd, None, mean, inv, gd, dg2, db2, ws, dxq3, 'lrelu', 0.2, beta=bd)
    assert np.array_equal(dxq3.numpy(), dxq.numpy()) and np.array_equal(dg1.numpy(), dg2.numpy())
    # ---- Theano bilinear x2 ----
    u1, u2 = dev.empty((N, C, 2 * H, 2 * W)), dev.empty((N, C, 2 * H, 2 * W))
    ops.upsample_bilinear2_fwd(xd, u1)
    wide, uq = qbuf((N, C, 2 * H, 2 * W))
    ops.upsample_bilinear2_fwd_q(xd, u2, uq)
    assert np.array_equal(u1.numpy(), u2.numpy())
    check_q(wide, uq, u1.numpy())
    wide2, uq2 = qbuf((N, C, 2 * H, 2 * W))
    ops.upsample_bilinear2_fwd_q(xd, None, uq2)
    assert np.array_equal(uq2.numpy(), uq.numpy())
    # ---- parity-planar -> interleaved ----
    pp = rng.randn(4 * N, C, H, W).astype(np.float32)
    ppd = dev.tensor(pp)
    h1, h2 = dev.empty((N, C, 2 * H, 2 * W)), dev.empty((N, C, 2 * H, 2 * W))
    ops.pp_to_hi(ppd, h1)
    wide, hq = qbuf((N, C, 2 * H, 2 * W))
    ops.pp_to_hi_q(ppd, h2, hq)
    assert np.array_equal(h1.numpy(), h2.numpy())
    check_q(wide, hq, h1.numpy())
    wide2, hq2 = qbuf((N, C, 2 * H, 2 * W))
    ops.pp_to_hi_q(ppd, None, hq2)
    assert np.array_equal(hq2.numpy(), hq.numpy())
    # ---- BatchNorm of a parity-planar tensor fused with the interleave (both directions) ----
    mean4, inv4 = dev.empty((1, C, 1, 1)), dev.empty((1, C, 1, 1))
    ops.bn_stats(ppd, mean4, inv4, ws)
    ypp = dev.empty(pp.shape)
    ops.bn_apply(ppd, ypp, mean4, inv4, gd, bd, 'relu', 0.0)
    ops.pp_to_hi(ypp, h1)
    wide, hq = qbuf((N, C, 2 * H, 2 * W))
    ops.bn_apply_hi(ppd, h2, hq, mean4, inv4, gd, bd, 'relu', 0.0)
    assert np.array_equal(h1.numpy(), h2.numpy())
    check_q(wide, hq, h1.numpy())
    wide2, hq2 = qbuf((N, C, 2 * H, 2 * W))
    ops.bn_apply_hi(ppd, None, hq2, mean4, inv4, gd, bd, 'relu', 0.0)
    assert np.array_equal(hq2.numpy(), hq.numpy())
    h3 = dev.zeros((N, C, 2 * H, 2 * W))
    ops.bn_apply_hi(ppd, h3, None, mean4, inv4, gd, bd, 'relu', 0.0)
    assert np.array_equal(h3.numpy(), h1.numpy())
    dhi = rng.randn(N, C, 2 * H, 2 * W).astype(np.float32)
    dhd = dev.tensor(dhi)
    dpp = dev.empty(pp.shape)
    ops.hi_to_pp(dhd, dpp)
    dxa, dxb = dev.empty(pp.shape), dev.empty(pp.shape)
    with tuning_env(GHM_NO_BN_SMALL="1"):
        ops.bn_backward_x(dpp, ppd, dxa, mean4, inv4, gd, bd, dg1, db1, ws, 'relu', 0.0)
    dxq = D.QTensor.empty(dev, pp.shape, dtype)
    ops.bn_backward_hi(dhd, ppd, dxb, dxq, mean4, inv4, gd, bd, dg2, db2, ws, 'relu', 0.0)
    assert rel(dxb.numpy(), dxa.numpy()) < 1e-6
    assert rel(dg2.numpy(), dg1.numpy()) < 1e-6 and rel(db2.numpy(), db1.numpy()) < 1e-6   # (another summation order)
    assert np.array_equal(dxq.numpy(), R(dxb.numpy()))
    dxq2 = D.QTensor.empty(dev, pp.shape, dtype)
    ops.bn_backward_hi(dhd, ppd, None, dxq2, mean4, inv4, gd, bd, dg2, db2, ws, 'relu', 0.0, accumulate=True)
    assert np.array_equal(dxq2.numpy(), dxq.numpy()) and rel(dg2.numpy(), 2 * dg1.numpy()) < 1e-6
    dxc = dev.zeros(pp.shape)
    ops.bn_backward_hi(dhd, ppd, dxc, None, mean4, inv4, gd, bd, dg2, db2, ws, 'relu', 0.0)
    assert np.array_equal(dxc.numpy(), dxb.numpy())
    # ---- backward of the fused conv + lrelu + 2x2 max-pool: full-resolution gradient from mask + pooled y + pooled dy ----
    Hf, Wf = 2 * H, 2 * W + 4                                   # (W % 4 == 0 for the plain kernel)
    Wp = Wf // 2
    m = rng.randint(1, 16, (N, C, H, Wp)).astype(np.uint8)
    yp = rng.randn(N, C, H, Wp).astype(np.float32)
    dyp = rng.randn(N, C, H, Wp).astype(np.float32)
    md = dev.alloc(m.size)
    dev.h2d(md, m)
    ypd, dypd = dev.tensor(yp), dev.tensor(dyp)
    f1, f2 = dev.empty((N, C, Hf, Wf)), dev.empty((N, C, Hf, Wf))
    ops.maxpool2_mask_bwd(md, ypd, dypd, f1, 'lrelu', 0.2)
    wide, fq = qbuf((N, C, Hf, Wf))
    gb = dev.zeros((1, C, 1, 1))
    ops.maxpool2_mask_bwd_q(md, ypd, dypd, f2, fq, 'lrelu', 0.2, gb)
    assert np.array_equal(f1.numpy(), f2.numpy())
    check_q(wide, fq, f1.numpy())
    assert rel(gb.numpy().ravel(), f1.numpy().astype(np.float64).sum(axis=(0, 2, 3))) < 1e-5
    wide2, fq2 = qbuf((N, C, Hf, Wf))
    ops.maxpool2_mask_bwd_q(md, ypd, dypd, None, fq2, 'lrelu', 0.2)
    assert np.array_equal(fq2.numpy(), fq.numpy())
