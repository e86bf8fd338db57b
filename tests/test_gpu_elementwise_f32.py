"""The fp32 pooling, resampling, loss, update and loss-scale kernels of csrc/elementwise.hip op by op, at the shapes of
tests/elementwise_f32_ref.py's tables (each row says which branch of its launcher it reaches; tests/test_elementwise_f32_ref.py
checks those claims, the inputs and the bounds on the CPU).

Per call:
  1. value: against the float64 definition, rel-L2 <= 1e-5 and per element |got - ref| <= k 2^-24 M (k, M:
     tests/elementwise_f32_ref.py); kernels that only move or select values (max-pool forward, nearest forward, max-pool
     backward with a linear or relu slope, axpby with b = 0) bit for bit; loss scalars within K_LOSS 2^-24 |loss|;
  2. nothing else is written: every tensor of the call, inputs included, is a view inside a NaN-canary-filled allocation
     (a whole tensor with a tail, a channel slice, or an odd offset / stride where the entry point takes a sample stride),
     no canary changes and the inputs are bit-unchanged;
  3. accumulate forms: the kernels here all finish the increment before they add the previous value (up_nearest_bwd,
     up_bilinear_bwd / bwd2, recon_loss's gradient, the loss scalar of scalar_loss / loss_final, bn_bwd_small / bn_bwd_final's
     dgamma and dbeta), so the result is exactly fl32(previous + increment), the increment being what the same call writes
     without accumulate.  dgamma / dbeta of an instance norm over several instances add one instance after the other, each
     rounded: they meet k_in_dgamma with the previous value inside M;
  4. no element and no row is left out of a comparison: ties, exact zeros and ignored borders are in the inputs on purpose.

rmsprop / adam over five launches, at n up to 2^24 + 3 and under the overflow contract are in tests/test_gpu_optimizers.py
(the two rules joined its machinery); here one launch of each is held to a per-element bound, and the host-side refusals.

Measured on the MI355X, max over all rows of |got - ref| / (2^-24 M) against the k asserted, the rel-L2, and the number of
comparisons (the module prints the three when it finishes; k of the libm ops is twice the measured worst, rounded up):
  maxpool2_fwd            bit-exact selection                                  -         4
  maxpool2_bwd            0.92 of 0 / 0 / 2 (linear, relu bit-exact / lrelu)   1.9e-09   16
  avgpool_fwd             1.68 of p p + 1 (5, 17, 65)                          1.4e-07   7
  avgpool_bwd             0 of 2                                               0         7
  nearest2_fwd            0 (a copy)                                           0         10
  nearest2_bwd            2.37 of 3 (4 accumulating; also exact fl32 sums)     5.7e-08   30
  bilinear2_fwd           1.60 of 4, against both definitions                  2.2e-08   20
  bilinear2_bwd           2.94 of 7 (8 accumulating; also exact fl32 sums)     6.2e-08   30
  lsgan_loss / _grad      0.85 of 4 / 1.95 of 5                                5.1e-08   30 / 18
  bce_loss / _grad        1.08 of 3 (libm) / 2.31 of 7                         6.4e-08   30 / 18
  recon_loss / _grad      0.50 of 4 / 1.80 of 4                                3.8e-08   45 / 27
  rmsprop acc / p         1.81 of 8 / 2.45 of 10                               3.6e-08   3 / 3
  adam m / v / p          < 2 of 6 / 1.87 of 7 / 2.74 of 6 (libm)              3.8e-08   6 each
  grad_check              the state bit for bit                                0         124
  loss_scale_update       the state bit for bit                                0         52
  instance_norm_fwd       2.99 of 6 / 6 / 7 (linear, relu / lrelu); tanh 2.85 of 6 (libm)   5.5e-08   24
  instance_norm mean, inv 0.99 of 2                                            3.2e-08   24
  instance_norm_bwd       3.45 of 15; tanh 2.94 of 6 (libm)                    7.1e-08   12
  instance_norm dgamma / dbeta   1.07 / 0.75 of 5 + instances                  6.2e-08   12 / 12
  axpby                   b = 0 bit-exact; 0.86 of 3 otherwise                 2.7e-08   8
No kernel needed a fix.  Of the 73 cases, the first run stopped at its 49th: 48 had passed and test_grad_check[1] failed on a
mistake of the test's own (it compared the state with a host copy of another shape); with that mended all 73 passed, the 24
that had not run included.  ghm_rmsprop gained the 16-byte alignment check its float4 loads rely on (refused on the host,
test_rmsprop_and_grad_check_refuse_misaligned_buffers).
Wall time on the MI355X, same run: this module 2.7 s (1.4 s in its tests), tests/test_gpu_elementwise_q.py 6.3 s.

ghm_maxpool2_mask_bwd(_bias) in fp32: tests/test_gpu_ops.py already reaches both forms of the bias variant --
test_conv_lrelu_maxpool_fused and four cases of test_conv_pool_backward_from_the_pooled_operands have per_plane % 256 == 0
(the in-kernel partial sums), the case (2, 32, 64, 72) has per_plane = 576 (two passes) -- so no row is added for it.
"""
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import GhmError
from tests import canary
from tests import elementwise_f32_ref as R

pytestmark = pytest.mark.gpu

A = R.ALPHA
_REF = {}
LEDGER = canary.Ledger(lambda op, w, r, n: "measured %-22s worst k %7.3f  rel-L2 %.2e  (%d comparisons)" % (op, w, r, n))
gpu, mem = canary.fixtures(LEDGER, _REF, loss_scale=True)
cached = functools.partial(canary.cached, _REF)
V, clean, unchanged, fl32_sum = canary.View.free, canary.clean, canary.unchanged, canary.fl32_sum
note, exact = LEDGER.note, LEDGER.exact


def scalar(t):
    return t.numpy().reshape(-1)[0]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,why", R.MAXPOOL_ROWS, ids=[str(s) for s, _ in R.MAXPOOL_ROWS])
def test_maxpool2(gpu, mem, shape, why):
    """ghm_maxpool2_fwd / _bwd on inputs whose windows tie in every pattern: the gradient goes to EVERY maximal position"""
    dev, ops, D = gpu
    N, C, H, W = shape
    ps = (N, C, H // 2, W // 2)
    d = cached(('maxpool', shape), lambda: R.maxpool_inputs(shape))
    x, y = V(gpu, shape, data=d['x']), V(gpu, ps)
    ops.maxpool2_fwd(x.t, y.t)
    y32 = y.numpy()
    LEDGER.tally('maxpool2_fwd')
    assert R.maxpool_selects(y32, d['x']), (shape, "an output is not an element of its window equal to the window's maximum")
    yref = R.maxpool_fwd(d['x'])
    assert np.array_equal(y32, yref)
    mixed = (R.windows(d['x']) == 0).any(-1) & (yref == 0)          # elsewhere the maximum has one bit pattern
    assert R.bits_equal(np.where(mixed, 0, y32), np.where(mixed, 0, yref.astype(np.float32)))
    unchanged(shape, x)
    clean(shape, y)
    dy = V(gpu, ps, data=d['dy'])
    yin = V(gpu, ps, data=yref)
    for act in R.ACTS:
        what = "%s %s" % (shape, act)
        ref, M = cached(('maxpool_bwd', shape, act), lambda: R.maxpool_bwd(d['x'], yref, d['dy'], act, A))
        dx = V(gpu, shape)
        ops.maxpool2_bwd(x.t, yin.t, dy.t, dx.t, act, A)
        got = dx.numpy()
        note('maxpool2_bwd', got, ref, M, what, k=R.K_MAXPOOL_BWD[act])
        if act == 'linear':
            exact('maxpool2_bwd', got, ref.astype(np.float32), what)
        elif act == 'relu':
            assert np.array_equal(got, ref), what
        clean(what, dx)
        unchanged(what, x, yin, dy)
        dev.free(dx.ptr)


@pytest.mark.parametrize("shape", R.MAXPOOL_REFUSED, ids=str)
def test_maxpool2_refuses_odd_sizes(gpu, mem, shape):
    """GHM_CHECK in the launchers: an error, and nothing launched"""
    dev, ops, D = gpu
    N, C, H, W = shape
    ps = (N, C, max(H // 2, 1), max(W // 2, 1))
    x, y, dy, dx = V(gpu, shape, data=np.ones(shape)), V(gpu, ps), V(gpu, ps, data=np.ones(ps)), V(gpu, shape)
    with pytest.raises(GhmError, match="even H, W"):
        ops.maxpool2_fwd(x.t, y.t)
    with pytest.raises(GhmError, match="even H, W"):
        ops.maxpool2_bwd(x.t, dy.t, dy.t, dx.t, 'linear', 0.0)
    dev.sync()
    for v in (y, dx):
        assert R.canary_changed(dev, v.ptr, 4 * v.total, np.zeros(2 * v.total, bool)).size == 0


@pytest.mark.parametrize("row,why", R.AVGPOOL_ROWS, ids=[str(r) for r, _ in R.AVGPOOL_ROWS])
def test_avgpool(gpu, mem, row, why):
    """ghm_avgpool_fwd / _bwd: p in {2, 4, 8}, global pooling, and H, W that p does not divide (border ignored / zero)"""
    dev, ops, D = gpu
    shape, p = row
    N, C, H, W = shape
    ps = (N, C, H // p, W // p)
    xin = cached(('view', shape), lambda: R.view_inputs(shape))['x']
    ref, M = R.avgpool_fwd(xin, p)
    x, y = V(gpu, shape, data=xin), V(gpu, ps)
    ops.avgpool_fwd(x.t, y.t, p)
    note('avgpool_fwd', y.numpy(), ref, M, str(row), k=R.k_avgpool_fwd(p))
    clean(row, y)
    unchanged(row, x)
    g = R.Q._rng(ps, 5).randn(*ps).astype(np.float32)
    dref, Md = R.avgpool_bwd(shape, g, p)
    dy, dx = V(gpu, ps, data=g), V(gpu, shape)
    ops.avgpool_bwd(dy.t, dx.t, p)
    got = dx.numpy()
    note('avgpool_bwd', got, dref, Md, str(row), k=R.K_AVGPOOL_BWD)
    border = np.ones(shape, bool)
    border[:, :, :H // p * p, :W // p * p] = False
    assert not got[border].any() and not np.signbit(got[border]).any(), (row, "the border is zero-filled")
    clean(row, dx)
    unchanged(row, dy)


@pytest.mark.parametrize("row,why", R.UP_ROWS, ids=["%s-%s" % (r[0], r[2]) for r, _ in R.UP_ROWS])
def test_upsample_nearest_and_bilinear(gpu, mem, row, why):
    """ghm_upsample_nearest2_fwd / _bwd and ghm_upsample_bilinear2_fwd / _bwd (both adjoint kernels), plain and accumulating,
    with the coarse source and the coarse gradient as strided views"""
    dev, ops, D = gpu
    shape, vx, vd, big = row
    N, C, H, W = shape
    fine = (N, C, 2 * H, 2 * W)
    what = "%s %s %s" % (shape, vd, R.bilinear_bwd_kernel(N, C, H, W, R.view_of(shape, vd))[0])
    d = cached(('up', shape), lambda: R.up_inputs(shape))
    x, g = V(gpu, shape, vx, d['x']), V(gpu, fine, data=d['g'])
    # forward
    y = V(gpu, fine)
    ops.upsample_nearest2_fwd(x.t, y.t)
    exact('nearest2_fwd', y.numpy(), R.nearest_fwd(d['x']), what)
    clean(what, y)
    y2 = V(gpu, fine)
    ops.upsample_bilinear2_fwd(x.t, y2.t)
    lit, closed, M = cached(('bil_fwd', shape), lambda: R.bilinear_fwd(d['x']))
    y32 = y2.numpy()
    note('bilinear2_fwd', y32, lit, M, what + " (Theano's algorithm)", k=R.K_BILINEAR_FWD)
    note('bilinear2_fwd', y32, closed, M, what + " (closed form)", k=R.K_BILINEAR_FWD)
    clean(what, y2)
    unchanged(what, x)
    for t in (y, y2):
        dev.free(t.ptr)
    # adjoints
    for op, fn, ref_fn, k in (('nearest2_bwd', ops.upsample_nearest2_bwd, R.nearest_bwd, R.K_NEAREST_BWD),
                              ('bilinear2_bwd', ops.upsample_bilinear2_bwd, R.bilinear_bwd, R.K_BILINEAR_BWD)):
        ref, Md = cached((op, shape), lambda: ref_fn(d['g']))
        dx = V(gpu, shape, vd)
        fn(g.t, dx.t)
        inc = dx.numpy()
        note(op, inc, ref, Md, what, k=k)
        clean(what, dx)
        dx.set(d['prev'])
        fn(g.t, dx.t, accumulate=True)
        acc = dx.numpy()
        exact(op, acc, fl32_sum(d['prev'], inc), what + " accumulate")
        note(op, acc, ref + d['prev'], Md + np.abs(d['prev']), what + " accumulate", k=k + 1)
        clean(what + " accumulate", dx)
        unchanged(what, g)
        dev.free(dx.ptr)


@pytest.mark.parametrize("kind", ['lsgan', 'bce'])
@pytest.mark.parametrize("n,why", R.LOSS_NS, ids=[str(n) for n, _ in R.LOSS_NS])
def test_scalar_losses(gpu, mem, n, why, kind):
    """ghm_lsgan_loss / ghm_bce_loss: one block, several blocks + loss_final_kernel, the capped grid; both targets, with and
    without a gradient buffer, grad_scale 0.5, accumulate_loss on the path the row takes, and a loss-scale state"""
    dev, ops, D = gpu
    fn = ops.lsgan_loss if kind == 'lsgan' else ops.bce_loss
    kl, kg = (R.K_LOSS, R.K_LSGAN_GRAD) if kind == 'lsgan' else (R.K_LIBM['bce_loss'], R.K_BCE_GRAD)
    data = cached(('loss', n, kind), lambda: R.loss_inputs(n, kind))
    d, grad, out = V(gpu, (n,), data=data), V(gpu, (n,)), V(gpu, (1,), data=[123.0])
    what = "%s n = %d (%s)" % (kind, n, R.loss_path(n))
    # target 1, gradient, grad_scale 0.5
    l1, Ml1, g1, Mg1 = R.scalar_loss(data, 1.0, kind, 0.5)
    fn(d.t, 1.0, out.t, grad.t, 0.5)
    got_l1, got_g1 = scalar(out), grad.numpy()
    note(kind + '_loss', [got_l1], [l1], [Ml1], what + " target 1", k=kl)
    note(kind + '_grad', got_g1.ravel(), g1.ravel(), Mg1.ravel(), what + " target 1", k=kg)
    clean(what, grad, out)
    unchanged(what, d)
    # target 0, no gradient buffer: the loss alone, then accumulated onto the first
    l0, Ml0, g0, Mg0 = R.scalar_loss(data, 0.0, kind, 1.0)
    out0 = V(gpu, (1,), data=[-7.0])
    fn(d.t, 0.0, out0.t, None, 1.0)
    got_l0 = scalar(out0)
    note(kind + '_loss', [got_l0], [l0], [Ml0], what + " target 0", k=kl)
    fn(d.t, 0.0, out.t, None, 1.0, accumulate_loss=True)
    exact(kind + '_loss', out.numpy(), fl32_sum([got_l1], [got_l0]).reshape(1, 1, 1, 1), what + " accumulate_loss")
    assert R.bits_equal(grad.numpy(), got_g1), (what, "grad = None must leave the earlier buffer alone")
    clean(what, grad, out, out0)
    # target 0 with a gradient
    fn(d.t, 0.0, out0.t, grad.t, 0.5)
    note(kind + '_grad', grad.numpy().ravel(), 0.5 * g0.ravel(), 0.5 * Mg0.ravel(), what + " target 0", k=kg)
    exact(kind + '_loss', out0.numpy(), np.float32(got_l0).reshape(1, 1, 1, 1), what + " same loss with a gradient")
    # a loss-scale state: the gradient times ls[0] (a power of two: exactly), the loss unscaled
    ls_host = np.array([2.0 ** 10, 2.0 ** -10, 5, 0, 2, 0, 0, 0], np.float32)
    ls = V(gpu, (8,), data=ls_host)
    dev.set_loss_scale_state(ls.t)
    try:
        fn(d.t, 1.0, out0.t, grad.t, 0.5)
        dev.sync()
    finally:
        dev.set_loss_scale_state(None)
    exact(kind + '_grad', grad.numpy(), got_g1 * np.float32(2.0 ** 10), what + " loss scale 2^10")
    exact(kind + '_loss', out0.numpy(), np.float32(got_l1).reshape(1, 1, 1, 1), what + " loss scale 2^10")
    unchanged(what, d, ls)
    clean(what, grad, out0)


@pytest.mark.parametrize("row,why", R.RECON_ROWS, ids=["%s-%s-%s" % (r[0], "l2" if r[1] else "l1", r[3]) for r, _ in R.RECON_ROWS])
def test_recon_loss(gpu, mem, row, why):
    """ghm_recon_loss: VEC 4 and VEC 1, a / b / grad with three different strides, L1 (sign(0) = 0) and L2, accumulate_grad,
    grad = None, the capped grid, a loss-scale state"""
    dev, ops, D = gpu
    shape, l2, va, vb, vg, gs = row
    what = "%s %s %s" % (shape, "l2" if l2 else "l1", why.split(":")[0])
    data = cached(('recon', shape), lambda: R.recon_inputs(shape))
    loss, gref, Mg = cached(('recon_ref', shape, l2, gs), lambda: R.recon_loss(data['a'], data['b'], l2, gs))
    a, b, g, out = V(gpu, shape, va, data['a']), V(gpu, shape, vb, data['b']), V(gpu, shape, vg), V(gpu, (1,), data=[55.0])
    ops.recon_loss(a.t, b.t, out.t, g.t, gs, l2=l2)
    got_l, inc = scalar(out), g.numpy()
    note('recon_loss', [got_l], [loss], [loss], what, k=R.K_LOSS)
    note('recon_grad', inc, gref, Mg, what, k=R.K_RECON_GRAD)
    eq = data['a'] == data['b']
    assert eq.any() and not inc[eq].any(), (what, "a == b must give a zero gradient")
    clean(what, g, out)
    # accumulate_grad: w is finished (a quotient) before the previous value is added
    g.set(data['prev'])
    ops.recon_loss(a.t, b.t, out.t, g.t, gs, l2=l2, accumulate_grad=True)
    exact('recon_grad', g.numpy(), fl32_sum(data['prev'], inc), what + " accumulate_grad")
    exact('recon_loss', out.numpy(), np.float32(got_l).reshape(1, 1, 1, 1), what + " accumulate_grad")
    # no gradient buffer
    out.set([-1.0])
    kept = g.numpy()
    ops.recon_loss(a.t, b.t, out.t, None, gs, l2=l2)
    assert R.bits_equal(g.numpy(), kept), (what, "grad = None must leave the earlier buffer alone")
    if R.recon_vec(shape[1], shape[2] * shape[3], R.view_of(shape, va), R.view_of(shape, vb), None) == \
            R.recon_vec(shape[1], shape[2] * shape[3], R.view_of(shape, va), R.view_of(shape, vb), R.view_of(shape, vg)):
        exact('recon_loss', out.numpy(), np.float32(got_l).reshape(1, 1, 1, 1), what + " grad = None")
    note('recon_loss', [scalar(out)], [loss], [loss], what + " grad = None", k=R.K_LOSS)
    # loss-scale state
    ls = V(gpu, (8,), data=np.array([2.0 ** 7, 2.0 ** -7, 0, 0, 0, 0, 0, 0], np.float32))
    dev.set_loss_scale_state(ls.t)
    try:
        ops.recon_loss(a.t, b.t, out.t, g.t, gs, l2=l2)
        dev.sync()
    finally:
        dev.set_loss_scale_state(None)
    exact('recon_grad', g.numpy(), inc * np.float32(2.0 ** 7), what + " loss scale 2^7")
    exact('recon_loss', out.numpy(), np.float32(got_l).reshape(1, 1, 1, 1), what + " loss scale 2^7")
    clean(what, g, out)
    unchanged(what, a, b, ls)


@pytest.mark.parametrize("n,why", R.OPT_NS, ids=[str(n) for n, _ in R.OPT_NS])
def test_rmsprop_and_adam_one_launch(gpu, mem, n, why):
    """ghm_rmsprop / ghm_adam from given states, non-default constants, grad_scale 0.5, element by element (float4 body and
    ragged tail alike); adam from t = 0 and from t = 10^5"""
    dev, ops, D = gpu
    d = R.opt_inputs(n)
    lr = 1e-2
    hyper = V(gpu, (2,), data=[lr, 0.0])
    p, g, acc = V(gpu, (n,), data=d['p']), V(gpu, (n,), data=d['g']), V(gpu, (n,), data=d['acc'])
    rho, eps = R.RMSPROP_CONSTS
    ops.rmsprop(p.t, g.t, acc.t, n, hyper.t, rho, eps, 0.5)
    p2, Mp, a2, Ma = R.rmsprop(d['p'], d['g'], d['acc'], lr, rho, eps, 0.5)
    note('rmsprop_acc', acc.numpy().ravel(), a2, Ma, "n = %d" % n, k=R.K_RMSPROP_ACC)
    note('rmsprop_p', p.numpy().ravel(), p2, Mp, "n = %d" % n, k=R.K_RMSPROP_P)
    assert R.rel(p.numpy().ravel() - d['p'], p2 - d['p']) <= R.REL_L2
    clean(n, p, acc)
    unchanged(n, g, hyper)
    b1, b2, eps = R.ADAM_CONSTS
    for t0 in R.ADAM_T0:
        hyper.set([lr, t0])
        p, m, v = V(gpu, (n,), data=d['p']), V(gpu, (n,), data=d['m']), V(gpu, (n,), data=d['acc'])
        ops.adam(p.t, g.t, m.t, v.t, n, hyper.t, b1, b2, eps, 0.5)
        p3, Mp, m3, Mm, v3, Mv = R.adam(d['p'], d['g'], d['m'], d['acc'], t0, lr, b1, b2, eps, 0.5)
        what = "n = %d t0 = %g" % (n, t0)
        note('adam_m', m.numpy().ravel(), m3, Mm, what, k=R.K_ADAM_M)
        note('adam_v', v.numpy().ravel(), v3, Mv, what, k=R.K_ADAM_V)
        note('adam_p', p.numpy().ravel(), p3, Mp, what, k=R.K_LIBM['adam_p'])
        assert R.rel(p.numpy().ravel() - d['p'], p3 - d['p']) <= R.REL_L2
        clean(what, p, m, v)
        unchanged(what, g, hyper)
        ops.adam_tick(hyper.t)
        assert hyper.numpy().ravel().tolist() == [np.float32(lr), t0 + 1]
        clean(what, hyper)


def test_rmsprop_and_grad_check_refuse_misaligned_buffers(gpu, mem):
    """the float4 kernels need 16-byte aligned buffers: the launchers refuse anything else on the host, before any launch"""
    dev, ops, D = gpu
    n = 64
    bufs = [V(gpu, (n,), data=np.ones(n)) for _ in range(3)]
    hyper = dev.tensor(np.array([1e-2, 0.0], np.float32))
    off = lambda v: D.DevTensor(dev, v.t.ptr + 4, (1, n - 1, 1, 1))
    for i in range(3):
        args = [off(b) if j == i else b.t for j, b in enumerate(bufs)]
        with pytest.raises(GhmError, match="16-byte aligned"):
            ops.rmsprop(args[0], args[1], args[2], n - 1, hyper)
    ls = V(gpu, (8,), data=np.zeros(8))
    dev.set_loss_scale_state(ls.t)
    try:
        with pytest.raises(GhmError, match="16-byte aligned"):
            ops.grad_check(off(bufs[0]), n - 1)
    finally:
        dev.set_loss_scale_state(None)
    with pytest.raises(GhmError, match="no loss-scale state"):
        ops.grad_check(bufs[0].t, n)
    with pytest.raises(GhmError, match="no loss-scale state"):
        ops.loss_scale_update()
    dev.sync()
    unchanged("refused", ls, *bufs)


@pytest.mark.parametrize("n,why", R.GRAD_CHECK_NS, ids=[str(n) for n, _ in R.GRAD_CHECK_NS])
def test_grad_check(gpu, mem, n, why):
    """ghm_grad_check: one non-finite value anywhere in [0, n) raises ls[3] and nothing else; finite extremes and the NaN
    canary right behind element n - 1 do not"""
    dev, ops, D = gpu
    rng = np.random.RandomState(n % 1000)
    base = rng.randn(n).astype(np.float32)
    base[rng.permutation(n)[:min(n, 6)]] = np.array(R.FINITE_EXTREMES, np.uint32).view(np.float32)[:min(n, 6)]
    g = V(gpu, (n,), data=base)
    ls_host = np.array([2.0 ** 12, 2.0 ** -12, 17, 0, 3, 0, 0, 0], np.float32)
    ls = V(gpu, (8,), data=ls_host)
    dev.set_loss_scale_state(ls.t)
    try:
        ops.grad_check(g.t, n)
        exact('grad_check', ls.numpy().ravel(), ls_host, "n = %d, finite values, a NaN canary from element n on" % n)
        if n >= 6:
            g.set(np.resize(np.array(R.FINITE_EXTREMES, np.uint32).view(np.float32), n))
            ops.grad_check(g.t, n)
            exact('grad_check', ls.numpy().ravel(), ls_host, "n = %d, finite extremes only" % n)
            g.set(base)
        raised = ls_host.copy()
        raised[3] = 1.0
        for pos in R.grad_check_positions(n):
            for bits in R.NONFINITE:
                dev.h2d(g.t.ptr + 4 * pos, np.array([bits], np.uint32))
                ops.grad_check(g.t, n)
                got = ls.numpy().ravel()
                dev.h2d(g.t.ptr + 4 * pos, base[pos:pos + 1])
                ls.t.set(ls_host)
                exact('grad_check', got, raised, "n = %d, 0x%08x at %d" % (n, bits, pos))
        # the flag stays up once raised
        ls.t.set(raised)
        ops.grad_check(g.t, n)
        exact('grad_check', ls.numpy().ravel(), raised, "n = %d, flag already set" % n)
        dev.sync()
    finally:
        dev.set_loss_scale_state(None)
    ls.data = raised
    unchanged(n, g, ls)


@pytest.mark.parametrize("run", range(len(R.LOSS_SCALE_RUNS)))
def test_loss_scale_update(gpu, mem, run):
    """ghm_loss_scale_update against the restated state machine, the overflow flag raised by ghm_grad_check itself"""
    dev, ops, D = gpu
    interval, lo, hi, s0, flags = R.LOSS_SCALE_RUNS[run]
    state = np.array([s0, 1 / s0, 0, 0, 0, 0, 0, 0], np.float32)
    ls = V(gpu, (8,), data=state)
    fine, inf = V(gpu, (5,), data=np.ones(5)), V(gpu, (5,), data=[1, 2, 3, 4, np.inf])
    dev.set_loss_scale_state(ls.t)
    try:
        for step, f in enumerate(flags):
            ops.grad_check((inf if f else fine).t, 5)
            state[3] = f
            exact('loss_scale_update', ls.numpy().ravel(), state, "step %d after the check" % step)
            if run == 0:
                ops.loss_scale_update(interval, lo, hi)
            else:
                ops.loss_scale_update()
            state = R.loss_scale_update(state, interval, lo, hi)
            got = ls.numpy().ravel()
            exact('loss_scale_update', got, state, "step %d, flag %d" % (step, f))
            assert got[1] == np.float32(1) / got[0] and got[3] == 0
        dev.sync()
    finally:
        dev.set_loss_scale_state(None)
    assert state[4] == sum(flags)
    clean(run, ls)
    unchanged(run, fine, inf)


@pytest.mark.parametrize("row,why", R.IN_ROWS, ids=["%s-g%d-%s" % (r[0], r[1], r[2]) for r, _ in R.IN_ROWS])
def test_instance_norm(gpu, mem, row, why):
    """Ops.instance_norm_fwd / _bwd: the one-launch kernels and the three-pass form, groups, slices, all four activations,
    dgamma / dbeta summed over the instances (written or accumulated)"""
    dev, ops, D = gpu
    shape, group, act, vx, vy, accumulate = row
    N, C, H, W = shape
    I = N // group
    what = "%s group %d %s (%s)" % (shape, group, act, why.split(":")[0])
    d = cached(('in', shape, group), lambda: R.in_inputs(shape, group))
    x, y = V(gpu, shape, vx, d['x']), V(gpu, shape, vy)
    mean, inv = V(gpu, (I, C, 1, 1)), V(gpu, (I, C, 1, 1))
    gamma, beta = V(gpu, (C,), data=d['gamma']), V(gpu, (C,), data=d['beta'])
    ws = dev.alloc(ops.bn_workspace(C))
    ops.instance_norm_fwd(x.t, y.t, mean.t, inv.t, gamma.t, beta.t, ws, R.IN_EPS, act, A, group)
    yref, M, mu, iv = cached(('in_fwd', shape, group, act), lambda: R.instance_norm_fwd(d['x'], d['gamma'], d['beta'], act, A, group))
    y32, m32, i32 = y.numpy(), mean.numpy().reshape(I, C), inv.numpy().reshape(I, C)
    if act == 'tanh':
        note('instance_norm_fwd/tanh', y32, yref, M, what, k=R.K_LIBM['in_fwd_tanh'])
    else:
        note('instance_norm_fwd', y32, yref, M, what, k=R.K_IN_FWD[act])
    # inv's rounding, and the fp64 cancellation E[x^2] - mu^2: two sums of up to 2^17 terms, 2^-36 of E[x^2] at most, which is
    # 2^-12 units of 2^-24
    var = 1 / iv ** 2
    note('instance_norm_stats', m32, mu, np.abs(mu) + 1e-30, what + " mean", k=R.K_IN_STATS)
    note('instance_norm_stats', i32, iv, iv * (1 + 2.0 ** -12 * (mu * mu + var) / var), what + " inv", k=R.K_IN_STATS)
    plane = y32[:group, C - 1]                                  # the constant instance: var = 0, inv = 1 / sqrt(eps), y = act(beta)
    want = R.Q.restate32_act(d['beta'][C - 1:], act, A)[0] if act != 'tanh' else plane.flat[0]
    exact('instance_norm_fwd', plane, np.full(plane.shape, want, np.float32), what + " constant plane")
    assert i32[0, C - 1] == np.float32(1 / np.sqrt(float(np.float32(R.IN_EPS)))) and m32[0, C - 1] == np.float32(0.75)
    mean.data, inv.data = mean.numpy(), inv.numpy()
    clean(what, y, mean, inv)
    unchanged(what, x, gamma, beta)
    # backward, from the statistics and the output the forward produced
    dout, dx = V(gpu, shape, data=d['dout']), V(gpu, shape, vy)
    dg, db = V(gpu, (C,), data=d['prev'][0]), V(gpu, (C,), data=d['prev'][1])
    ops.instance_norm_bwd(dout.t, x.t, dx.t, mean.t, inv.t, gamma.t, beta.t, dg.t, db.t, ws, act, A, accumulate, group)
    ref, Mx, dgr, Mg, dbr, Mb = R.instance_norm_bwd(d['dout'], y32, d['x'], m32, i32, d['gamma'], act, A, group)
    note('instance_norm_bwd/tanh' if act == 'tanh' else 'instance_norm_bwd', dx.numpy(), ref, Mx, what,
         k=R.K_LIBM['in_bwd_tanh'] if act == 'tanh' else R.K_IN_BWD)
    prev = d['prev'].astype(np.float64) if accumulate else np.zeros((2, C))
    kg = R.k_in_dgamma(I) + (R.K_LIBM['in_bwd_tanh'] if act == 'tanh' else 0)
    got_g, got_b = dg.numpy().ravel(), db.numpy().ravel()
    note('instance_norm_dgamma', got_g, dgr + prev[0], Mg + np.abs(prev[0]), what + (" accumulate" if accumulate else ""), k=kg)
    note('instance_norm_dbeta', got_b, dbr + prev[1], Mb + np.abs(prev[1]), what + (" accumulate" if accumulate else ""), k=kg)
    clean(what, dx, dg, db)
    unchanged(what, x, dout, gamma, beta, mean, inv)
    if I == 1 and accumulate:           # one instance: fl32(previous + increment) exactly
        dg.set(np.zeros(C)), db.set(np.zeros(C))
        ops.instance_norm_bwd(dout.t, x.t, dx.t, mean.t, inv.t, gamma.t, beta.t, dg.t, db.t, ws, act, A, False, group)
        exact('instance_norm_dgamma', got_g, fl32_sum(d['prev'][0], dg.numpy().ravel()), what + " exact accumulate")
        exact('instance_norm_dbeta', got_b, fl32_sum(d['prev'][1], db.numpy().ravel()), what + " exact accumulate")


def test_instance_norm_refuses_partial_groups(gpu, mem):
    dev, ops, D = gpu
    shape, group = R.IN_REFUSED
    N, C, H, W = shape
    x, y, dx = V(gpu, shape, data=np.ones(shape)), V(gpu, shape), V(gpu, shape)
    stat = [V(gpu, (2, C, 1, 1), data=np.ones((2, C))) for _ in range(2)]
    par = [V(gpu, (C,), data=np.ones(C)) for _ in range(4)]
    ws = dev.alloc(ops.bn_workspace(C))
    with pytest.raises(GhmError, match="whole groups"):
        ops.instance_norm_fwd(x.t, y.t, stat[0].t, stat[1].t, par[0].t, par[1].t, ws, R.IN_EPS, 'linear', 0.0, group)
    with pytest.raises(GhmError, match="whole groups"):
        ops.instance_norm_bwd(x.t, x.t, dx.t, stat[0].t, stat[1].t, par[0].t, par[1].t, par[2].t, par[3].t, ws, 'linear', 0.0, False, group)
    dev.sync()
    for v in (y, dx):
        assert R.canary_changed(dev, v.ptr, 4 * v.total, np.zeros(2 * v.total, bool)).size == 0
    unchanged("refused", x, *(stat + par))


@pytest.mark.parametrize("n", [1, 255, 256, 1003])
def test_axpby_with_b_zero_does_not_read_y(gpu, mem, n):
    """ghm_axpby: b == 0 means y is write-only -- over a NaN-filled y the result is a x exactly; b != 0 reads it"""
    dev, ops, D = gpu
    xin = R.view_inputs((1, 1, 1, n))['x'].ravel()
    xin[0] = -0.0
    x, y = V(gpu, (n,), data=xin), V(gpu, (n,))
    ops.axpby(0.3, x.t, 0.0, y.t, n)
    exact('axpby', y.numpy().ravel(), R.axpby_b0(0.3, xin), "n = %d, b = 0" % n)
    prev = y.numpy().ravel()
    ops.axpby(2.0, x.t, -0.5, y.t, n)
    ref = 2.0 * xin.astype(np.float64) - 0.5 * prev
    note('axpby', y.numpy().ravel(), ref, np.abs(2.0 * xin) + np.abs(0.5 * prev), "n = %d, b = -0.5" % n, k=3)
    clean(n, y)
    unchanged(n, x)
