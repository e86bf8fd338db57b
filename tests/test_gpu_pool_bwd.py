"""The pooled block's gradient kernels (Conv2D 5x5 'same' -> activation -> MaxPool2D(2), whose full-resolution gradient is
rebuilt inside the kernels from the pooled gradient, the pooled activation and the 4-bit arg-max mask with its sign bit)
through device.Ops, per element and inside canary views, at the rows of tests/pool_bwd_ref.py (tests/test_pool_bwd_ref.py
checks the rows' claims, the inputs and the bounds on the CPU):
  pool_thin_wgrad_kernel<8, U, KPW> + pool_thin_wgrad_final and pool_thin_dgrad_kernel (csrc/conv_pool_bwd.hip),
  maxpool2_mask_bwd_compress_kernel (csrc/elementwise_q.hip) and sp_wgrad_pooled_kernel<64 | 32, 3 | 2> (csrc/conv_split.hip).

x, dx and the q tensors xq, dyq, cq live in views (whole / channel slice of a wider buffer / offset start) inside NaN-canary
allocations; gp, yp, the mask, dW, db, the packed weights, both workspaces, idx and flags are buffers of EXACTLY the documented
size with 4 KB of canary in front and behind, in the same allocation.
  1. integer pass, every row: dW, db, dx equal float64 bit for bit in lrelu 0.25, relu and linear, with yp and with the
     slope from the mask's sign bit, without db, accumulating onto integers; cq's pieces, every idx word and every flags int
     (flags pre-filled with garbage) equal the reference; the sparse-instruction result equals float64 AND the dense
     conv2d_wgrad_lp_q bit for bit in the five flag patterns.
  2. real pass: |got - ref| <= k 2^-24 M per element and the bound of the older tests; a repeated call, the call without yp,
     every served (GHM_POOLW_U, GHM_POOLW_KPW) pair and the XCD remap on / off give identical bits; an unserved pair is an error
     that writes nothing; accumulate is exactly fl32(previous + increment) -- pool_thin_wgrad_final ``(accumulate ? *o : 0.f)
     + v``, pool_thin_dgrad_kernel ``r0.x += p0.x`` on the finished sum, sp_wgrad_pooled_kernel ``v.x += w.x`` on the finished
     accumulator and ghm_reduce_splits all add the previous value last (read in the source).
  3. no canary changes, the inputs stay bit-unchanged, the outputs are finite, and the results are the same bits when
     everything outside the views and buffers is repainted with a second, finite pattern.
  4. refusals that write nothing: the data gradient at K = 65, at an odd x_nstride and at a dx 4 bytes off 8-byte alignment.

Measured on the MI355X (the module prints this when it finishes): the worst |got - ref| / (2^-24 M) over all rows and calls
against the asserted k, the older tests' measure (rel-L2, bound 1e-5; the split modes max |got - ref| / max |ref|, bounds 2e-6
and 3e-5) and the number of comparisons, bit-exact ones included:
  wgrad (dW, db)   1.771 of  4   rel-L2        3.93e-07   (631)
  dgrad (dx)       6.719 of 14   rel-L2        4.40e-07   (116)
  bf16x3 pooled    6.333 of 22   max-abs/scale 6.96e-07   (675)     bf16x3 dense   5.642 of 22   6.96e-07   (25)
  bf16x2 pooled    4.065 of 22   max-abs/scale 4.43e-07   (600)     bf16x2 dense   4.065 of 22   5.02e-07   (25)
Wall time on the MI355X: 78 tests in 3.3 s (2.5 s between the fixture's start and end).  The two fp32 families' worst equal
the CPU restatement's to the digit (1.771, 6.719): it is the kernels' own summation order.

What was found: nothing to fix.  Every integer comparison was bit-exact in every row, activation and flag pattern, with yp and
with the sign bit; cq, every idx word and every flags int matched; the sparse instruction returned the dense split kernel's and
float64's bits; every repeated call, every served (U, KPW) pair and the XCD remap on / off gave identical bits; every
accumulate was exactly fl32(previous + increment); every refusal left its outputs untouched; no canary changed.
sp_wgrad_pooled_kernel does NOT need the 256 bytes that the older test and the engine allocate behind idx and flags: with both
buffers at exactly the documented size (N K/8 H W/32 units of 16 bytes; N H ints) no guard was written, and the results are
the same bits whether the bytes behind them hold NaNs or finite values -- its index loads are masked to CT x 4 x NCH lanes and
its flag reads to rows below i_end.  The sizes in include/ghm.h stand as documented; no library source changed.
"""
import ctypes as C

import numpy as np
import pytest

from gan_heightmaps_amd._lib import GhmError, call, load, tuning_env
from tests import canary
from tests import pool_bwd_ref as R

pytestmark = pytest.mark.gpu

POOLW_PAIRS = [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (2, 2)]


def family(key):
    """'bf16x3 pooled' -> 'bf16x3': the bound and the second figure of a key are those of its first word"""
    return key.split()[0]


LEDGER = canary.Ledger(lambda key, w, r, n: "measured %-14s worst k %7.3f of %2d  %s %.2e  (%d comparisons)"
                       % (key, w, R.K_BOUND[family(key)], "max-abs/scale" if family(key) in R.MAXABS else "rel-L2", r, n),
                       bound=lambda key: R.K_BOUND[family(key)], rel_limit=lambda key: R.MAXABS.get(family(key), R.REL_L2),
                       maxabs=lambda key: family(key) in R.MAXABS, describe=lambda name, i, shape: R.border_class(name, shape, i))
gpu, mem = canary.fixtures(LEDGER, {})
V, Buf, QV = canary.View.named, canary.Bytes, canary.QView.named
clean, unchanged, repaint, note, exact = canary.clean, canary.unchanged, canary.repaint, LEDGER.note, LEDGER.exact


# ---- the sparse fp32 gradients ----
class Sparse:
    """the operands of one (N, H, W, K) row on the device"""

    def __init__(self, gpu, g, view, d, kind):
        self.gpu, self.g, self.view, self.d, self.kind = gpu, g, view, d, kind
        dev, ops, D = gpu
        N, H, W, K = g
        self.sp = (N, K, H // 2, W // 2)
        self.mask, self.gp, self.yp = Buf(gpu, np.prod(self.sp), d['mask']), Buf(gpu, 4 * np.prod(self.sp), d['gp']), Buf(gpu, 4 * np.prod(self.sp), d['yp'])
        self.inputs = [self.mask, self.gp, self.yp]
        self.buffers = []
        xns = R.view_layout((N, 1, H, W), view)[1]
        self.desc = D.conv_desc(N, 1, H, W, K, 5, 5, 1, 2, xns)
        if kind == 'wgrad':
            self.x = V(gpu, (N, 1, H, W), view, d['x'])
            assert self.x.t.nstride == xns
            self.ws = Buf(gpu, ops.pool_wgrad_sparse_workspace(self.desc))
            self.inputs.append(self.x)
            self.buffers.append(self.ws)
        else:
            self.w = Buf(gpu, 4 * 25 * K, D.pack_conv_w(d['W']))
            self.inputs.append(self.w)

    def wgrad(self, act, alpha, yp=True, db=True, prev=False, accumulate=False):
        """-> (dW [K, 1, 5, 5], db [K] or None, the two output buffers)"""
        dev, ops, D = self.gpu
        K = self.g[3]
        dw = Buf(self.gpu, 4 * 25 * K, D.pack_conv_w(self.d['prev_dW']) if prev else None)
        dbb = Buf(self.gpu, 4 * K, self.d['prev_db'] if prev else None)
        ops.conv2d_pool_wgrad_sparse(self.desc, self.x.t, self.mask.ptr, self.yp.tensor(self.sp) if yp else None, self.gp.tensor(self.sp),
                                     dw.ptr, dbb.ptr if db else None, self.ws.ptr, act, alpha, accumulate)
        return D.unpack_conv_w(dw.numpy(), K, 1, 5, 5), (dbb.numpy() if db else None), [dw, dbb]

    def out(self, prev=False, view=None):
        N, H, W, K = self.g
        return V(self.gpu, (N, 1, H, W), view or self.view, self.d['prev_dx'] if prev else None)

    def dgrad(self, o, act, alpha, yp=True, accumulate=False):
        self.gpu[1].conv2d_pool_dgrad_sparse(self.desc, self.mask.ptr, self.yp.tensor(self.sp) if yp else None, self.gp.tensor(self.sp),
                                             self.w.ptr, o.t, act, alpha, accumulate)
        return o.numpy()

    def settle(self, what, outs):
        unchanged(what, *self.inputs)
        clean(what, *(self.buffers + outs))

    def everything(self, outs):
        return self.inputs + self.buffers + outs


def sparse_inputs(kind, g, integer, forward):
    if forward:
        return R.forward_inputs(g, integer)
    return R.inputs(g, (R.wgrad_seams if kind == 'wgrad' else R.dgrad_seams)(g), integer)


def args_of(d, yp, act, alpha):
    return (d['mask'], d['yp'] if yp else None, d['gp'], act, alpha)


WG_CASES = [(r, False) for r in R.WGRAD_ROWS] + [(r, True) for r in R.WGRAD_ROWS if r.g in R.WGRAD_FORWARD]
DG_CASES = [(r, False) for r in R.DGRAD_ROWS] + [(r, True) for r in R.DGRAD_ROWS if r.g in R.DGRAD_FORWARD]
case_id = lambda c: R.row_id(c[0]) + ("-forward" if c[1] else "")


@pytest.mark.parametrize("case", WG_CASES, ids=case_id)
def test_weight_gradient_row(gpu, mem, case):
    row, forward = case
    g, key = row.g, 'wgrad'
    # ---- integer pass ----
    d = sparse_inputs('wgrad', g, True, forward)
    p, outs = Sparse(gpu, g, row.view, d, 'wgrad'), []
    for act in R.ACTS:
        for yp in (True, False):
            ref = R.ref(d['x'], d['W'], *args_of(d, yp, act, R.SLOPE))
            dW, db, o = p.wgrad(act, R.SLOPE, yp=yp)
            what = "integers, %s, %s" % (act, "yp" if yp else "sign bit")
            exact(key, dW, ref['dW'], "dW " + what, at='dW', zero_sign=act != 'relu')
            exact(key, db, ref['db'], "db " + what, at='db', zero_sign=act != 'relu')
            outs += o
    dW0, _, o = p.wgrad('lrelu', R.SLOPE, db=False)
    exact(key, dW0, ref_of(d, 'lrelu', R.SLOPE)['dW'], "dW integers, no db", at='dW')
    assert o[1].untouched(), "db was written though none was asked for"
    outs += o
    dW, db, o = p.wgrad('lrelu', R.SLOPE, prev=True, accumulate=True)
    exact(key, dW, d['prev_dW'] + ref_of(d, 'lrelu', R.SLOPE)['dW'], "dW integers, accumulate", at='dW')
    exact(key, db, d['prev_db'] + ref_of(d, 'lrelu', R.SLOPE)['db'], "db integers, accumulate", at='db')
    p.settle((case_id(case), "integer pass"), outs + o)
    # ---- real pass ----
    d = sparse_inputs('wgrad', g, False, forward)
    p, outs = Sparse(gpu, g, row.view, d, 'wgrad'), []
    first = None
    for act in R.ACTS:
        a = args_of(d, True, act, R.ALPHA)
        ref, M = R.ref(d['x'], d['W'], *a), R.magnitude(d['x'], d['W'], *a)
        dW, db, o = p.wgrad(act, R.ALPHA)
        note(key, dW, ref['dW'], M['dW'], "dW real, " + act, at='dW')
        note(key, db, ref['db'], M['db'], "db real, " + act, at='db')
        outs += o
        dW2, db2, o = p.wgrad(act, R.ALPHA, yp=False)
        exact(key, dW2, dW, "dW real, %s: the sign bit gives the bits of yp" % act, at='dW')
        exact(key, db2, db, "db real, %s: the sign bit gives the bits of yp" % act, at='db')
        outs += o
        first = first or (dW, db)
    dW, db = first
    dW2, db2, o = p.wgrad('lrelu', R.ALPHA)
    exact(key, dW2, dW, "dW real, repeated call", at='dW')
    exact(key, db2, db, "db real, repeated call", at='db')
    outs += o
    dW3, db3, o = p.wgrad('lrelu', R.ALPHA, prev=True, accumulate=True)
    exact(key, dW3, (d['prev_dW'] + dW).astype(np.float32), "dW real, accumulate == fl32(previous + increment)", at='dW')
    exact(key, db3, (d['prev_db'] + db).astype(np.float32), "db real, accumulate == fl32(previous + increment)", at='db')
    outs += o
    p.settle((case_id(case), "real pass"), outs)
    repaint(gpu[0], *p.everything([]))
    dW4, db4, o = p.wgrad('lrelu', R.ALPHA)
    exact(key, dW4, dW, "dW real, a second pattern outside the views", at='dW')
    exact(key, db4, db, "db real, a second pattern outside the views", at='db')


def ref_of(d, act, alpha, yp=True):
    return R.ref(d['x'], d['W'], *args_of(d, yp, act, alpha))


def test_weight_gradient_launch_shapes_give_the_same_bits(gpu, mem):
    """U and KPW change the launch shape, not the summation order"""
    key = 'wgrad'
    for row in [r for r in R.WGRAD_ROWS if r.g in ((2, 8, 32, 9), (1, 46, 32, 17), (1, 2, 2172, 8), (1, 4, 128, 65), (1, 4, 262, 8))]:
        d = sparse_inputs('wgrad', row.g, False, False)
        p = Sparse(gpu, row.g, row.view, d, 'wgrad')
        dW, db, outs = p.wgrad('lrelu', R.ALPHA)
        for u, kpw in POOLW_PAIRS:
            with tuning_env(GHM_POOLW_U=str(u), GHM_POOLW_KPW=str(kpw)):
                dW2, db2, o = p.wgrad('lrelu', R.ALPHA)
            exact(key, dW2, dW, "dW %s U %d KPW %d" % (R.row_id(row), u, kpw), at='dW')
            exact(key, db2, db, "db %s U %d KPW %d" % (R.row_id(row), u, kpw), at='db')
            outs += o
        p.settle((R.row_id(row), "launch shapes"), outs)


def test_weight_gradient_unserved_pair_and_width_write_nothing(gpu, mem):
    dev, ops, D = gpu
    row = R.WGRAD_ROWS[0]
    d = sparse_inputs('wgrad', row.g, False, False)
    p = Sparse(gpu, row.g, row.view, d, 'wgrad')
    K = row.g[3]
    dw, dbb = Buf(gpu, 4 * 25 * K), Buf(gpu, 4 * K)
    with tuning_env(GHM_POOLW_U='3', GHM_POOLW_KPW='2'):
        with pytest.raises(GhmError, match="no variant"):
            ops.conv2d_pool_wgrad_sparse(p.desc, p.x.t, p.mask.ptr, p.yp.tensor(p.sp), p.gp.tensor(p.sp), dw.ptr, dbb.ptr, p.ws.ptr, 'lrelu', R.ALPHA)
    dev.sync()
    assert dw.untouched() and dbb.untouched()
    N, H, W, K = R.WGRAD_UNSERVED
    dn = D.conv_desc(N, 1, H, W, K, 5, 5, 1, 2)
    assert ops.pool_bwd_sparse_supported(dn, 'lrelu') & 1 == 0 and ops.pool_wgrad_sparse_workspace(dn) == 0
    with pytest.raises(GhmError, match="not served"):
        ops.conv2d_pool_wgrad_sparse(dn, p.x.t, p.mask.ptr, None, p.gp.tensor(p.sp), dw.ptr, dbb.ptr, p.ws.ptr, 'lrelu', R.ALPHA)
    dev.sync()
    assert dw.untouched() and dbb.untouched()
    p.settle("refusals", [dw, dbb])


@pytest.mark.parametrize("case", DG_CASES, ids=case_id)
def test_data_gradient_row(gpu, mem, case):
    row, forward = case
    g, key = row.g, 'dgrad'
    N, H, W, K = g
    d = sparse_inputs('dgrad', g, True, forward)
    p, outs = Sparse(gpu, g, row.view, d, 'dgrad'), []
    for act in R.ACTS:
        for yp in (True, False):
            outs.append(p.out())
            exact(key, p.dgrad(outs[-1], act, R.SLOPE, yp=yp), ref_of(d, act, R.SLOPE, yp)['dx'],
                  "dx integers, %s, %s" % (act, "yp" if yp else "sign bit"), at='dx', zero_sign=act != 'relu')
    outs.append(p.out(prev=True))
    exact(key, p.dgrad(outs[-1], 'lrelu', R.SLOPE, accumulate=True), d['prev_dx'] + ref_of(d, 'lrelu', R.SLOPE)['dx'],
          "dx integers, accumulate", at='dx')
    if N >= 2:      # one sample of the batch, as the generator's step asks for the fake half
        dev, ops, D = gpu
        o = p.out()
        one, per = D.conv_desc(1, 1, H, W, K, 5, 5, 1, 2, o.t.nstride), int(np.prod(p.sp[1:]))
        ops.conv2d_pool_dgrad_sparse(one, p.mask.ptr + per, p.yp.tensor((1,) + p.sp[1:], per), p.gp.tensor((1,) + p.sp[1:], per), p.w.ptr,
                                     o.t.samples(1, 2), 'lrelu', R.SLOPE)
        got = o.numpy()
        exact(key, got[1:2], ref_of(d, 'lrelu', R.SLOPE)['dx'][1:2], "dx integers, sample 1 alone", at='dx')
        assert np.isnan(got[0]).all() and (N == 2 or np.isnan(got[2:]).all()), "another sample was written"
        outs.append(o)
    p.settle((case_id(case), "integer pass"), outs)
    d = sparse_inputs('dgrad', g, False, forward)
    p, outs = Sparse(gpu, g, row.view, d, 'dgrad'), []
    first = None
    for act in R.ACTS:
        a = args_of(d, True, act, R.ALPHA)
        ref, M = R.ref(d['x'], d['W'], *a), R.magnitude(d['x'], d['W'], *a)
        outs += [p.out(), p.out()]
        dx = p.dgrad(outs[-2], act, R.ALPHA)
        note(key, dx, ref['dx'], M['dx'], "dx real, " + act, at='dx')
        exact(key, p.dgrad(outs[-1], act, R.ALPHA, yp=False), dx, "dx real, %s: the sign bit gives the bits of yp" % act, at='dx')
        first = dx if first is None else first
    outs += [p.out(), p.out(prev=True)]
    exact(key, p.dgrad(outs[-2], 'lrelu', R.ALPHA), first, "dx real, repeated call", at='dx')
    exact(key, p.dgrad(outs[-1], 'lrelu', R.ALPHA, accumulate=True), (d['prev_dx'] + first).astype(np.float32),
          "dx real, accumulate == fl32(previous + increment)", at='dx')
    p.settle((case_id(case), "real pass"), outs)
    o = p.out()
    repaint(gpu[0], *p.everything([o]))
    exact(key, p.dgrad(o, 'lrelu', R.ALPHA), first, "dx real, a second pattern outside the views", at='dx')


def test_data_gradient_refusals_write_nothing(gpu, mem):
    dev, ops, D = gpu
    g = R.DGRAD_REFUSED_K
    N, H, W, K = g
    d = R.inputs(g, R.dgrad_seams(g), False)
    p = Sparse(gpu, g, 'whole', d, 'dgrad')
    assert ops.pool_bwd_sparse_supported(p.desc, 'lrelu') == 1
    o = p.out()
    with pytest.raises(GhmError, match="not served"):
        p.dgrad(o, 'lrelu', R.ALPHA)
    g = R.DGRAD_ROWS[1].g
    N, H, W, K = g
    d = R.inputs(g, R.dgrad_seams(g), False)
    q = Sparse(gpu, g, 'whole', d, 'dgrad')
    o2, o3 = q.out(), q.out(view='off4')
    q.desc = D.conv_desc(N, 1, H, W, K, 5, 5, 1, 2, H * W + 1)
    assert ops.pool_bwd_sparse_supported(q.desc, 'lrelu') == 1                 # bit 1 clear at an odd sample stride
    with pytest.raises(GhmError, match="not served"):
        q.dgrad(o2, 'lrelu', R.ALPHA)
    q.desc = D.conv_desc(N, 1, H, W, K, 5, 5, 1, 2)
    assert o3.t.ptr % 8 == 4
    with pytest.raises(GhmError, match="8-byte aligned"):
        q.dgrad(o3, 'lrelu', R.ALPHA)
    dev.sync()
    for v in (o, o2, o3):
        assert np.isnan(v.numpy()).all(), "a refused call wrote into dx"
    p.settle("refused, K = 65", [o])
    q.settle("refused, stride and alignment", [o2, o3])


# ---- compress + the sparse matrix instruction ----
SPLIT_VIEWS = [('slice', 'offset', 'whole'), ('offset', 'whole', 'slice'), ('whole', 'slice', 'offset')]       # (xq, dyq, cq) by row


def split_ws_bytes(d):
    n = C.c_size_t()
    call("ghm_conv2d_wgrad_split_workspace", C.byref(d), C.byref(n))
    return n.value


class Split:
    """x as a q tensor, the mask and the pooled gradient of one (N, C, K, H, W) row; ``produce`` runs the two max-pool
    backwards (dense q tensor, compressed form) for one activation"""

    def __init__(self, gpu, g, mode, d, views):
        self.gpu, self.g, self.mode, self.d, self.views = gpu, g, mode, d, views
        dev, ops, D = gpu
        N, Cc, K, H, W = g
        self.sp = (N, K, H // 2, W // 2)
        self.desc = D.conv_desc(N, Cc, H, W, K, 5, 5, 1, 2)
        self.xq = QV(gpu, (N, Cc, H, W), mode, views[0])
        ops.q_pack(dev.tensor(d['x']), self.xq.q)
        self.xq.snapshot()
        self.mask, self.gp, self.yp = Buf(gpu, np.prod(self.sp), d['mask']), Buf(gpu, 4 * np.prod(self.sp), d['gp']), Buf(gpu, 4 * np.prod(self.sp), d['yp'])
        self.ws = Buf(gpu, split_ws_bytes(self.desc))
        self.inputs = [self.xq, self.mask, self.gp, self.yp]

    def produce(self, act, alpha, yp):
        dev, ops, D = self.gpu
        N, Cc, K, H, W = self.g
        ypt = self.yp.tensor(self.sp) if yp else None
        self.dyq, self.dense = QV(self.gpu, (N, K, H, W), self.mode, self.views[1]), V(self.gpu, (N, K, H, W), 'whole')
        ops.maxpool2_mask_bwd_q(self.mask.ptr, ypt, self.gp.tensor(self.sp), self.dense.t, self.dyq.q, act, alpha)
        self.cq = QV(self.gpu, (N, K, H, W // 2), self.mode, self.views[2])
        self.idx = Buf(self.gpu, N * (K // 8) * H * (W // 32) * 16)
        self.flags = Buf(self.gpu, N * H * 4, np.full(N * H, 0x5a5a5a5a, np.int32))
        ops.maxpool2_mask_bwd_compress_q(self.mask.ptr, ypt, self.gp.tensor(self.sp), self.cq.q, self.idx.ptr, self.flags.ptr, act, alpha)
        for t in (self.dyq, self.cq):
            t.snapshot()
        self.idx.data, self.flags.data = self.idx.bytes(), self.flags.bytes()
        self.produced = [self.dyq, self.cq, self.idx, self.flags]
        return self.cq.pieces(), self.idx.bytes().view(np.uint16), self.flags.bytes().view(np.int32)

    def check_compressed(self, key, act, alpha, yp, what):
        N, Cc, K, H, W = self.g
        cq, idx, flags = self.produce(act, alpha, yp)
        wq, widx, wflags = R.compressed(self.d['mask'], self.d['yp'] if yp else None, self.d['gp'], act, alpha, self.mode)
        for i, (have, want) in enumerate(zip(cq, wq)):
            exact(key, have, want, "cq %s: cq piece %d" % (what, i), at='cq', zero_sign=act != 'relu')
        assert np.array_equal(idx, widx.reshape(-1)), (what, "%d idx words differ" % (idx != widx.reshape(-1)).sum())
        assert np.array_equal(flags, wflags), (what, "flags", flags.reshape(N, H), wflags.reshape(N, H))
        G32 = R.dense_grad(self.d['mask'], self.d['yp'] if yp else None, self.d['gp'], act, alpha, np.float32)
        exact(key, self.dense.numpy(), G32, "G %s: the dense gradient" % what, at='G', zero_sign=act != 'relu')
        clean(what, self.dense, *self.produced)
        LEDGER.tally(key, 2)
        return G32

    def dense_wgrad(self):
        dev, ops, D = self.gpu
        N, Cc, K, H, W = self.g
        o = Buf(self.gpu, 4 * Cc * 25 * K)
        ops.conv2d_wgrad_lp_q(self.desc, self.xq.q, self.dyq.q, o.ptr, self.ws.ptr, self.mode)
        return D.unpack_conv_w(o.numpy(), K, Cc, 5, 5), o

    def pooled_wgrad(self, prev=None, accumulate=False):
        dev, ops, D = self.gpu
        N, Cc, K, H, W = self.g
        o = Buf(self.gpu, 4 * Cc * 25 * K, None if prev is None else D.pack_conv_w(prev))
        ops.conv2d_wgrad_pooled_split(self.desc, self.xq.q, self.dyq.q, self.cq.q, self.idx.ptr, self.flags.ptr, o.ptr, self.ws.ptr, self.mode, accumulate)
        return D.unpack_conv_w(o.numpy(), K, Cc, 5, 5), o

    def settle(self, what, outs):
        unchanged(what, *(self.inputs + self.produced))
        clean(what, self.ws, *outs)


SPLIT_CASES = [(i, mode, pattern) for i in range(len(R.SPLIT_ROWS)) for mode in R.SPLIT_MODES for pattern in R.FLAG_PATTERNS]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "%s-%s-%s" % (R.row_id(R.SPLIT_ROWS[c[0]]), c[1], c[2]))
def test_compress_and_sparse_instruction_row(gpu, mem, case):
    i, mode, pattern = case
    row, key = R.SPLIT_ROWS[i], mode + " pooled"
    g = row.g
    dev, ops, D = gpu
    with tuning_env(**row.env):
        plan = R.split_plan(g, row.env, dev.info()['num_cu'])
        assert plan == {k: row.reaches[k] for k in plan}, "this device plans the row differently"
        assert ops.wgrad_pooled_split_supported(D.conv_desc(g[0], g[1], g[3], g[4], g[2], 5, 5, 1, 2), mode)
        # ---- integer pass ----
        d = R.split_inputs(g, plan, pattern, True)
        p = Split(gpu, g, mode, d, SPLIT_VIEWS[i % 3])
        acts = [(a, y) for a in R.ACTS for y in (True, False)] if pattern == 'alternate' else [('lrelu', True)]
        for act, yp in acts[::-1]:                          # (lrelu with yp last: the weight gradient below runs on it)
            G32 = p.check_compressed(key, act, R.SLOPE, yp, "integers, %s, %s" % (act, "yp" if yp else "sign bit"))
        want = R.wgrad64(d['x'], G32)
        a, oa = p.dense_wgrad()
        b, ob = p.pooled_wgrad()
        exact(key, a, want, "dW integers: the dense split kernel == float64", at='dW')
        exact(key, b, want, "dW integers: the sparse instruction == float64", at='dW')
        with tuning_env(GHM_SPLIT_WGRAD_NO_XCD='1'):
            b2, ob2 = p.pooled_wgrad()
        exact(key, b2, want, "dW integers, no XCD remap", at='dW')
        b3, ob3 = p.pooled_wgrad(prev=d['prev_dW'], accumulate=True)
        exact(key, b3, d['prev_dW'] + want, "dW integers, accumulate", at='dW')
        p.settle((case, "integer pass"), [oa, ob, ob2, ob3])
        # ---- real pass ----
        d = R.split_inputs(g, plan, pattern, False)
        p = Split(gpu, g, mode, d, SPLIT_VIEWS[i % 3])
        G32 = p.check_compressed(key, 'lrelu', R.ALPHA, False, "real, lrelu, sign bit")
        ref, M = R.ref_split(mode, d['x'], G32), R.wgrad64(np.abs(d['x']), np.abs(G32))
        a, oa = p.dense_wgrad()
        b, ob = p.pooled_wgrad()
        note(mode + " dense", a, ref, M, "dW real", at='dW')
        note(key, b, ref, M, "dW real", at='dW')
        b1, ob1 = p.pooled_wgrad()
        exact(key, b1, b, "dW real, repeated call", at='dW')
        with tuning_env(GHM_SPLIT_WGRAD_NO_XCD='1'):
            b2, ob2 = p.pooled_wgrad()
        exact(key, b2, b, "dW real, no XCD remap", at='dW')
        b3, ob3 = p.pooled_wgrad(prev=d['prev_dW'], accumulate=True)
        exact(key, b3, (d['prev_dW'] + b).astype(np.float32), "dW real, accumulate == fl32(previous + increment)", at='dW')
        p.settle((case, "real pass"), [oa, ob, ob1, ob2, ob3])
        # the same bits with another pattern outside every view and buffer: the 256 bytes the older test and the engine add
        # behind idx and flags are not read into a result
        repaint(dev, *(p.inputs + p.produced + [p.ws]))
        b4, ob4 = p.pooled_wgrad()
        exact(key, b4, b, "dW real, a second pattern outside the views", at='dW')


def test_no_sparse_wgrad_switch_says_no(gpu):
    dev, ops, D = gpu
    N, Cc, K, H, W = R.SPLIT_ROWS[1].g
    d = D.conv_desc(N, Cc, H, W, K, 5, 5, 1, 2)
    assert ops.wgrad_pooled_split_supported(d, 'bf16x3')
    with tuning_env(GHM_NO_SPARSE_WGRAD='1'):
        assert not ops.wgrad_pooled_split_supported(d, 'bf16x3') and load().ghm_conv2d_wgrad_pooled_split_supported(C.byref(d)) == 0
