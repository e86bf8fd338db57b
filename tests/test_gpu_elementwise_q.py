"""The element-wise q producers (csrc/elementwise_q.hip) op by op, in the four q dtypes ('bf16', 'f16' and the split dtypes
'bf16x3', 'bf16x2'), in both kernel forms behind GHM_Q_TWO_PIXELS / GHM_POOLBWD_WINDOWS, at the shapes of
tests/elementwise_q_ref.py's tables (each row says which branch of the dispatch code it reaches;
tests/test_elementwise_q_ref.py checks those claims and the bounds on the CPU).

Per call:
  1. value: the fp32 output against the float64 definition, rel-L2 <= 1e-5 and per element |got - ref| <= k 2^-24 M
     (k, M: tests/elementwise_q_ref.py);
  2. every piece plane of the q copy is, bit for bit, pieces(fp32 output, dtype); for 'bf16x3' the pieces sum to the fp32 output;
  3. the pieces equal those ghm_split_pack / ghm_q_pack write for the same fp32 tensor;
  4. with the fp32 pointer NULL the q planes are bit-identical;
  5. nothing else is written: the q targets are channel slices in the middle of a wider buffer, or whole allocations with a
     tail behind the last plane, filled with a NaN canary beforehand; the fp32 outputs likewise where the entry point takes a
     sample stride (a tail behind them where it does not); fp32 inputs are slices of canary-filled buffers too;
  6. dgamma / dbeta / dbias against float64 (rel-L2 <= 1e-5); accumulate=True gives exactly fl32(previous + increment);
  7. the second kernel form agrees with the default one (q planes and fp32 bit-identical; the BatchNorm backward's fp32
     within the per-element bound).

Measured on the MI355X, max over all rows, dtypes, activations and output forms of |got - ref| / (2^-24 M) against the k
asserted, and of the rel-L2 (the module prints both when it finishes):
  bn_apply_q           2.64 of 4 / 5 / 8 (linear, relu / lrelu / tanh)   4.3e-08
  bn_apply_hi          2.59 of 4 / 5 / 8                                 4.1e-08
  bn_backward_q        3.57 of 15 (the same in the two-pixel form)       1.2e-07
  bn_backward_hi       3.57 of 15                                        1.2e-07
  bilinear2_fwd_q      1.75 of 4                                         2.4e-08
  pp_to_hi_q           0 (a copy)                                        0
  maxpool2_mask_bwd_q  0.95 of 2                                         5.0e-09
No entry point needed a fix: all 148 cases passed on their first run.
"""
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import tuning_env
from tests import canary
from tests import elementwise_q_ref as R

pytestmark = pytest.mark.gpu

A = R.ALPHA
_REF = {}
LEDGER = canary.Ledger(lambda op, w, r, n: "measured %-18s worst k %.3f  rel-L2 %.2e" % (op, w, r))
gpu, mem = canary.fixtures(LEDGER, _REF)
cached = functools.partial(canary.cached, _REF)
F32, Q = canary.View.framed, canary.QView.framed
note, clean = LEDGER.note, canary.clean


def check_q(gpu, qt, out32, dtype, what):
    """assertions 2, 3 and 5 for one q target"""
    dev, ops, D = gpu
    got, exp = qt.pieces(), R.pieces(out32, dtype)
    for p in range(qt.planes):
        if not R.bits_equal(got[p], exp[p]):
            bad = np.argwhere(got[p].view(np.uint32) != exp[p].view(np.uint32))
            pytest.fail("%s: piece %d differs from pieces(fp32 output) at %d elements, first (n, c, y, x) = %s: stored %r, expected %r"
                        % (what, p, len(bad), tuple(bad[0]), got[p][tuple(bad[0])], exp[p][tuple(bad[0])]))
    if dtype == 'bf16x3':       # (equal as numbers: the pieces of -0.0 are -0.0, +0.0, +0.0)
        assert np.array_equal(sum(g.astype(np.float64) for g in got), out32.astype(np.float64)), what
    packed = Q(gpu, out32.shape, dtype, 'whole')
    src = dev.tensor(out32)
    ops.q_pack(src, packed.q)
    for p, pk in enumerate(packed.pieces()):
        assert R.bits_equal(got[p], pk), (what, "piece %d differs from the device's pack of the same tensor" % p)
    s = qt.stray()
    assert s.size == 0, (what, "%d halfwords outside the q view were written, first at unit %d (view: %d units from unit %d, samples %d "
                         "and planes %d units apart)" % (s.size, s[0] // 8 if s.size else -1, qt.q.Cc // 8 * qt.q.HW,
                                                         (qt.q.ptr - qt.ptr) // 16, qt.q.nstride, qt.q.pstride))
    for t in (packed.ptr, src.ptr):
        dev.free(t)


def same_planes(a, b, what):
    for p, (u, v) in enumerate(zip(a.pieces(), b.pieces())):
        assert R.bits_equal(u, v), (what, "piece %d" % p)
    s = b.stray()
    assert s.size == 0, (what, "%d stray halfwords, first %d" % (s.size, s[0] if s.size else -1))


def vec(dev, a):
    return dev.tensor(np.asarray(a, np.float32))


def acts_for(shape, acts):
    return acts if np.prod(shape) <= R.BIG else acts[:1]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.BN_ROWS, ids=[str(s) for s, _ in R.BN_ROWS])
def test_bn_apply_q(gpu, mem, shape, why, dtype):
    """ghm_bn_apply_q: default and GHM_Q_TWO_PIXELS form; fp32 + q into slices, q only into a whole tensor"""
    dev, ops, D = gpu
    d = cached(('bn', shape), lambda: R.bn_inputs(shape))
    x = F32(gpu, shape, 'slice', d['x'])
    mean, inv, gd, bd = (vec(dev, d[k]) for k in ('mean', 'inv', 'gamma', 'beta'))
    for act in acts_for(shape, R.ACTS + ('tanh',)):
        what = "%s %s %s" % (shape, dtype, act)
        ref, M = cached(('bn_apply', shape, act), lambda: R.bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, A))
        y, q = F32(gpu, shape, 'slice'), Q(gpu, shape, dtype, 'slice')
        ops.bn_apply_q(x.t, y.t, mean, inv, gd, bd, q.q, act, A)
        y32 = y.t.numpy()
        note('bn_apply_q', y32, ref, M, what, k=R.K_BN_APPLY[act])
        check_q(gpu, q, y32, dtype, what)
        clean(what, y)
        q2 = Q(gpu, shape, dtype, 'whole')
        ops.bn_apply_q(x.t, None, mean, inv, gd, bd, q2.q, act, A)
        same_planes(q, q2, what + " q only")
        y3, q3 = F32(gpu, shape, 'slice'), Q(gpu, shape, dtype, 'slice')
        with tuning_env(GHM_Q_TWO_PIXELS="1"):
            ops.bn_apply_q(x.t, y3.t, mean, inv, gd, bd, q3.q, act, A)
        assert R.bits_equal(y3.t.numpy(), y32), what + " two pixels"
        same_planes(q, q3, what + " two pixels")
        clean(what + " two pixels", y3)
        for t in (y, q, q2, y3, q3):
            dev.free(t.ptr)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.BN_ROWS, ids=[str(s) for s, _ in R.BN_ROWS])
def test_bn_backward_q(gpu, mem, shape, why, dtype):
    """ghm_bn_backward_q (reductions of ghm_bn_backward_sums + the apply pass in both forms): with y, and with y recomputed"""
    dev, ops, D = gpu
    C = shape[1]
    d = cached(('bn', shape), lambda: R.bn_inputs(shape))
    x, dout = F32(gpu, shape, 'slice', d['x']), F32(gpu, shape, 'slice', d['dout'])
    mean, inv, gd, bd = (vec(dev, d[k]) for k in ('mean', 'inv', 'gamma', 'beta'))
    ws = dev.alloc(ops.bn_workspace(C))
    prev = np.random.RandomState(7).randn(2, C).astype(np.float32)
    for act in acts_for(shape, R.ACTS):
        what = "%s %s %s" % (shape, dtype, act)
        yd = F32(gpu, shape, 'slice')
        ops.bn_apply(x.t, yd.t, mean, inv, gd, bd, act, A)
        y32 = cached(('bn_y32', shape, act), lambda: yd.t.numpy())
        assert R.bits_equal(yd.t.numpy(), y32)
        ref, M, dg_ref, db_ref = cached(('bn_bwd', shape, act),
                                        lambda: R.bn_backward(d['dout'], y32, d['x'], d['mean'], d['inv'], d['gamma'], act, A))
        dx, q = F32(gpu, shape, 'slice'), Q(gpu, shape, dtype, 'slice')
        dg, db = dev.zeros((1, C, 1, 1)), dev.zeros((1, C, 1, 1))
        ops.bn_backward_q(dout.t, yd.t, x.t, dx.t, mean, inv, gd, dg, db, ws, q.q, act, A)
        dx32 = dx.t.numpy()
        note('bn_backward_q', dx32, ref, M, what, k=R.K_BN_BWD)
        check_q(gpu, q, dx32, dtype, what)
        clean(what, dx)
        inc_g, inc_b = dg.numpy().ravel(), db.numpy().ravel()
        print("%s: dgamma rel-L2 %.2e dbeta rel-L2 %.2e" % (what, R.rel(inc_g, dg_ref), R.rel(inc_b, db_ref)))
        assert R.rel(inc_g, dg_ref) <= R.REL_L2 and R.rel(inc_b, db_ref) <= R.REL_L2, what
        # q only, y recomputed from x (the form the step issues), accumulating into the parameter gradients
        q2 = Q(gpu, shape, dtype, 'whole')
        dg.set(prev[0]), db.set(prev[1])
        ops.bn_backward_q(dout.t, None, x.t, None, mean, inv, gd, dg, db, ws, q2.q, act, A, accumulate=True, beta=bd)
        same_planes(q, q2, what + " q only, y recomputed")
        assert R.bits_equal(dg.numpy().ravel(), canary.fl32_sum(prev[0], inc_g)) and R.bits_equal(db.numpy().ravel(), canary.fl32_sum(prev[1], inc_b)), what
        # two pixels per thread
        dx3, q3 = F32(gpu, shape, 'slice'), Q(gpu, shape, dtype, 'slice')
        with tuning_env(GHM_Q_TWO_PIXELS="1"):
            ops.bn_backward_q(dout.t, yd.t, x.t, dx3.t, mean, inv, gd, dg, db, ws, q3.q, act, A)
        dx3_32 = dx3.t.numpy()
        note('bn_backward_q/px2', dx3_32, ref, M, what, k=R.K_BN_BWD)
        check_q(gpu, q3, dx3_32, dtype, what + " two pixels")
        same_planes(q, q3, what + " two pixels")
        clean(what + " two pixels", dx3)
        assert R.bits_equal(dg.numpy().ravel(), inc_g) and R.bits_equal(db.numpy().ravel(), inc_b)
        for t in (yd, dx, q, q2, dx3, q3):
            dev.free(t.ptr)
    for t in (x, dout):
        clean("inputs", t)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.COARSE_ROWS, ids=[str(s) for s, _ in R.COARSE_ROWS])
def test_bilinear_and_interleave_q(gpu, mem, shape, why, dtype):
    """ghm_upsample_bilinear2_fwd_q and ghm_pp_to_hi_q at coarse maps down to 1x1"""
    dev, ops, D = gpu
    N, C, H, W = shape
    fine = (N, C, 2 * H, 2 * W)
    what = "%s %s" % (shape, dtype)
    xin = cached(('bn', shape), lambda: R.bn_inputs(shape))['x']
    ref, M = cached(('bilinear', shape), lambda: R.bilinear(xin))
    x = F32(gpu, shape, 'slice', xin)
    y, q = F32(gpu, fine, 'whole'), Q(gpu, fine, dtype, 'slice')
    ops.upsample_bilinear2_fwd_q(x.t, y.t, q.q)
    y32 = y.t.numpy()
    note('bilinear2_fwd_q', y32, ref, M, what, k=R.K_BILINEAR)
    check_q(gpu, q, y32, dtype, what)
    clean(what, y)
    q2 = Q(gpu, fine, dtype, 'whole')
    ops.upsample_bilinear2_fwd_q(x.t, None, q2.q)
    same_planes(q, q2, what + " q only")
    # the interleave: a permutation, exact
    pp = cached(('hi', shape), lambda: R.hi_inputs(shape))['x']
    ppd = dev.tensor(pp)
    h, hq = F32(gpu, fine, 'slice'), Q(gpu, fine, dtype, 'slice')
    ops.pp_to_hi_q(ppd, h.t, hq.q)
    h32 = h.t.numpy()
    hi_ref = R.pp_to_hi(pp)
    note('pp_to_hi_q', h32, hi_ref.astype(np.float64), np.abs(hi_ref).astype(np.float64), what, k=R.K_INTERLEAVE)
    assert R.bits_equal(h32, hi_ref)
    check_q(gpu, hq, h32, dtype, what + " interleave")
    clean(what + " interleave", h)
    hq2 = Q(gpu, fine, dtype, 'whole')
    ops.pp_to_hi_q(ppd, None, hq2.q)
    same_planes(hq, hq2, what + " interleave, q only")


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.COARSE_ROWS, ids=[str(s) for s, _ in R.COARSE_ROWS])
def test_bn_apply_hi(gpu, mem, shape, why, dtype):
    """ghm_bn_apply_hi: fp32 + q, q only, fp32 only"""
    dev, ops, D = gpu
    N, C, H, W = shape
    fine = (N, C, 2 * H, 2 * W)
    d = cached(('hi', shape), lambda: R.hi_inputs(shape))
    ppd = dev.tensor(d['x'])
    mean, inv, gd, bd = (vec(dev, d[k]) for k in ('mean', 'inv', 'gamma', 'beta'))
    for act in acts_for(fine, R.ACTS + ('tanh',)):
        what = "%s %s %s" % (shape, dtype, act)
        ref, M = cached(('bn_apply_hi', shape, act), lambda: R.bn_apply_hi(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, A))
        h, q = F32(gpu, fine, 'slice'), Q(gpu, fine, dtype, 'slice')
        ops.bn_apply_hi(ppd, h.t, q.q, mean, inv, gd, bd, act, A)
        h32 = h.t.numpy()
        note('bn_apply_hi', h32, ref, M, what, k=R.K_BN_APPLY[act])
        check_q(gpu, q, h32, dtype, what)
        clean(what, h)
        q2 = Q(gpu, fine, dtype, 'whole')
        ops.bn_apply_hi(ppd, None, q2.q, mean, inv, gd, bd, act, A)
        same_planes(q, q2, what + " q only")
        h3 = F32(gpu, fine, 'whole')
        ops.bn_apply_hi(ppd, h3.t, None, mean, inv, gd, bd, act, A)
        assert R.bits_equal(h3.t.numpy(), h32), what + " fp32 only"
        clean(what + " fp32 only", h3)
        for t in (h, q, q2, h3):
            dev.free(t.ptr)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.HI_BWD_ROWS, ids=[str(s) for s, _ in R.HI_BWD_ROWS])
def test_bn_backward_hi(gpu, mem, shape, why, dtype):
    """ghm_bn_backward_hi: the multi-block partial sums of bn_bwd_hi_partial and the apply pass; fp32 + q, q only, fp32 only"""
    dev, ops, D = gpu
    N, K, H, W = shape
    ppshape, fine = (4 * N, K, H, W), (N, K, 2 * H, 2 * W)
    d = cached(('hi', shape), lambda: R.hi_inputs(shape))
    ppd = dev.tensor(d['x'])
    dhi = F32(gpu, fine, 'slice', d['dhi'])
    mean, inv, gd, bd = (vec(dev, d[k]) for k in ('mean', 'inv', 'gamma', 'beta'))
    ws = dev.alloc(ops.bn_workspace(K))
    prev = np.random.RandomState(8).randn(2, K).astype(np.float32)
    for act in acts_for(ppshape, R.ACTS):
        what = "%s %s %s" % (shape, dtype, act)
        yd = dev.empty(ppshape)
        ops.bn_apply(ppd, yd, mean, inv, gd, bd, act, A)
        y32 = cached(('hi_y32', shape, act), lambda: yd.numpy())
        ref, M, dg_ref, db_ref = cached(('bn_bwd_hi', shape, act),
                                        lambda: R.bn_backward_hi(d['dhi'], y32, d['x'], d['mean'], d['inv'], d['gamma'], act, A))
        dx, q = F32(gpu, ppshape, 'whole'), Q(gpu, ppshape, dtype, 'whole')
        dg, db = dev.zeros((1, K, 1, 1)), dev.zeros((1, K, 1, 1))
        ops.bn_backward_hi(dhi.t, ppd, dx.t, q.q, mean, inv, gd, bd, dg, db, ws, act, A)
        dx32 = dx.t.numpy()
        note('bn_backward_hi', dx32, ref, M, what, k=R.K_BN_BWD)
        check_q(gpu, q, dx32, dtype, what)
        clean(what, dx)
        inc_g, inc_b = dg.numpy().ravel(), db.numpy().ravel()
        print("%s: dgamma rel-L2 %.2e dbeta rel-L2 %.2e" % (what, R.rel(inc_g, dg_ref), R.rel(inc_b, db_ref)))
        assert R.rel(inc_g, dg_ref) <= R.REL_L2 and R.rel(inc_b, db_ref) <= R.REL_L2, what
        q2 = Q(gpu, ppshape, dtype, 'whole')
        dg.set(prev[0]), db.set(prev[1])
        ops.bn_backward_hi(dhi.t, ppd, None, q2.q, mean, inv, gd, bd, dg, db, ws, act, A, accumulate=True)
        same_planes(q, q2, what + " q only")
        assert R.bits_equal(dg.numpy().ravel(), canary.fl32_sum(prev[0], inc_g)) and R.bits_equal(db.numpy().ravel(), canary.fl32_sum(prev[1], inc_b)), what
        dx3 = F32(gpu, ppshape, 'whole')
        ops.bn_backward_hi(dhi.t, ppd, dx3.t, None, mean, inv, gd, bd, dg, db, ws, act, A)
        assert R.bits_equal(dx3.t.numpy(), dx32), what + " fp32 only"
        clean(what + " fp32 only", dx3)
        for t in (dx, q, q2, dx3):
            dev.free(t.ptr)
        dev.free(yd.ptr)
    clean("dhi", dhi)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape,why", R.POOL_ROWS, ids=[str(s) for s, _ in R.POOL_ROWS])
def test_maxpool2_mask_bwd_q(gpu, mem, shape, why, dtype):
    """ghm_maxpool2_mask_bwd_q: a thread per fine column (default) and per window pair (GHM_POOLBWD_WINDOWS); the slope from y
    and from the mask's sign bit; the bias gradient summed over N * bpp per-block partials"""
    dev, ops, D = gpu
    N, C, H, W = shape
    d = cached(('pool', shape), lambda: R.pool_inputs(shape))
    md = dev.alloc(d['mask'].size)
    dev.h2d(md, d['mask'])
    ypd, dypd = dev.tensor(d['y']), dev.tensor(d['dy'])
    prev = np.random.RandomState(9).randn(C).astype(np.float32)
    for act in acts_for(shape, R.ACTS):
        for with_y in (True, False):
            what = "%s %s %s %s" % (shape, dtype, act, "y" if with_y else "sign bit")
            yarg = ypd if with_y else None
            ref, M, db_ref = cached(('pool', shape, act, with_y),
                                    lambda: R.mask_bwd(d['mask'], d['y'] if with_y else None, d['dy'], act, A))
            dx, q = F32(gpu, shape, 'whole'), Q(gpu, shape, dtype, 'slice')
            gb = dev.zeros((1, C, 1, 1))
            ops.maxpool2_mask_bwd_q(md, yarg, dypd, dx.t, q.q, act, A, gb)
            dx32 = dx.t.numpy()
            note('maxpool2_mask_bwd_q', dx32, ref, M, what, k=R.K_MASK_BWD)
            check_q(gpu, q, dx32, dtype, what)
            clean(what, dx)
            inc = gb.numpy().ravel()
            print("%s: dbias rel-L2 %.2e" % (what, R.rel(inc, db_ref)))
            assert R.rel(inc, db_ref) <= R.REL_L2, what
            if not with_y:          # q only (what the step issues), accumulating into the bias gradient
                q2 = Q(gpu, shape, dtype, 'whole')
                gb.set(prev)
                ops.maxpool2_mask_bwd_q(md, None, dypd, None, q2.q, act, A, gb, accumulate=True)
                same_planes(q, q2, what + " q only")
                assert R.bits_equal(gb.numpy().ravel(), canary.fl32_sum(prev, inc)), what
                dev.free(q2.ptr)
            dx3, q3 = F32(gpu, shape, 'whole'), Q(gpu, shape, dtype, 'slice')
            with tuning_env(GHM_POOLBWD_WINDOWS="1"):
                ops.maxpool2_mask_bwd_q(md, yarg, dypd, dx3.t, q3.q, act, A, gb)
            assert R.bits_equal(dx3.t.numpy(), dx32), what + " windows"
            same_planes(q, q3, what + " windows")
            clean(what + " windows", dx3)
            assert R.rel(gb.numpy().ravel(), db_ref) <= R.REL_L2, what + " windows"
            for t in (dx, q, dx3, q3):
                dev.free(t.ptr)
            dev.free(gb.ptr)
