"""The 3x3 stride-2 pad-1 convolutions (forward, data gradient, weight gradient) through device.Ops in the five arithmetic
modes, per element and inside canary views, at the rows of tests/conv_s2_ref.py (each row names the tile, wave form and split
path it reaches; tests/test_conv_s2_ref.py checks those claims, the inputs and the bound on the CPU).

Per row, under the row's tuning environment:
  1. integer pass: inputs of small integers (every partial sum in any order below 2^24, every operand exact in bf16 and fp16,
     second and third split pieces zero) -- the result equals the float64 answer BIT FOR BIT: plain, with bias + leaky relu
     0.25, with bias + relu (there a zero of either sign: see ``exact``), accumulating onto a known integer tensor, and the forms with the producer's activation backward
     in the epilogue (slope 0.25 and relu, activation operand with both signs and exact zeros).  All tiles and split counts
     of a geometry are held to the same bits, so they agree with each other;
  2. real pass: |got - ref| <= k 2^-24 M per element (k, M: tests/conv_s2_ref.py) and the rel-L2 bound of the older tests; a
     repeated call gives identical bits; the accumulate form is exactly fl32(previous + increment), the increment being what
     the same call writes without accumulate -- every kernel of this family, single-pass or split-K (igemm_splitk_epilogue,
     sm_finish_kernel, reduce_splits*), finishes its sum (and bias) before it adds the previous value, so none needs the
     bound with |previous| inside M;
  3. nothing else is written and nothing outside a view is read: x, dy, y, dx, the activation operand and the bias live in
     views (whole / channel slice of a wider buffer / offset start) inside NaN-canary allocations with 4 KB in front and
     behind, the packed weights, dW and the weight-gradient workspace are whole buffers with a canary head and tail; no canary
     changes, the inputs are bit-unchanged, the output is finite;
  4. q operands (two rows per mode, single-pass plans): the q output equals pieces(fp32 output of the same call) bit for bit,
     the call with q inputs equals the call with fp32 inputs bit for bit, canaries round the q tensors.

Measured on the MI355X (the module prints this table when it finishes): max over all rows and calls of |got - ref| / (2^-24 M)
against the asserted k, the rel-L2 (bounds 1e-5 fp32, 2e-5 bf16 / f16 against the rounded operands, 2e-6 split), and the number
of comparisons (bit-exact ones included):
            forward                       data gradient                 weight gradient
  f32       5.78 of 13  2.6e-07  (35)     5.92 of 10  1.2e-07  (44)     3.26 of 11  3.6e-07  (20)
  bf16      2.44 of  9  9.3e-08  (38)     2.66 of  7  7.3e-08  (37)     1.56 of 10  1.1e-07  (15)
  f16       2.21 of 12  1.0e-07  (38)     3.08 of 14  7.8e-08  (37)     1.30 of  8  1.2e-07  (15)
  bf16x3    5.52 of 44  1.4e-07  (54)     3.45 of 21  7.2e-08  (42)     3.30 of 22  1.8e-07  (15)
  bf16x2    5.06 of 39  1.4e-07  (53)     3.06 of 20  7.2e-08  (41)     2.48 of 22  1.3e-07  (15)
(the split kernels' separate leading and correction accumulators sit far inside the single-accumulator restatement their k
comes from.)  Every integer comparison was bit-exact in every mode, tile and split count, every accumulate form exactly
fl32(previous + increment), every repeated call bit-identical, no canary changed and no result depended on bytes outside an
input view: no kernel needed a fix.  The first run failed on two mistakes of the module's own: it expected relu(v) = +0 for a
negative v where the epilogues that fold relu into a slope return v * 0 = -0 (and the reverse), which ``exact`` now treats as
the same zero for relu alone; and a failure message that did not format.  Wall time on the MI355X: 74 tests in 1.8 s (1.1 s
between the fixture's start and end).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import load, tuning_env
from tests import canary
from tests import conv_s2_ref as R
from tests import elementwise_q_ref as Q

pytestmark = pytest.mark.gpu

_REF = {}
LEDGER = canary.Ledger(lambda key, w, r, n: "measured %-7s %-6s worst k %7.3f of %2d  rel-L2 %.2e  (%d comparisons)" % (key + (w, R.K_BOUND[key], r, n)),
                       bound=R.K_BOUND.__getitem__, rel_limit=lambda key: R.REL_L2[key[0]], describe=lambda kind, i, shape: R.parity_class(kind, i))
gpu, mem = canary.fixtures(LEDGER, _REF)
cached = functools.partial(canary.cached, _REF)
V, Raw, QV = canary.View.named, canary.Bytes.rounded, canary.QView.named
clean, unchanged, note, exact = canary.clean, canary.unchanged, LEDGER.note, LEDGER.exact


def act64(v, act):
    if act == 'relu':
        return np.where(v > 0, v, 0.0)
    return v if act == 'linear' else np.where(v > 0, v, R.SLOPE * v)


def slope64(y, act):
    return np.where(np.asarray(y) > 0, 1.0, R.SLOPE if act == 'lrelu' else 0.0)


class Product:
    """the operands of one row on the device, and its calls"""

    def __init__(self, gpu, mode, kind, g, view, d):
        self.gpu, self.mode, self.kind, self.g, self.view, self.d = gpu, mode, kind, g, view, d
        dev, ops, D = gpu
        N, C, H, W, K = g
        xs, ws, ys = R.shapes(g)
        self.fam = R.family(mode)
        self.x, self.dy = V(gpu, xs, view, d['x']), V(gpu, ys, view, d['dy'])
        self.desc = D.conv_desc(N, C, H, W, K, 3, 3, 2, 1, self.x.t.nstride, self.dy.t.nstride)
        self.inputs, self.buffers = [self.x, self.dy], []
        self.wp = Raw(gpu, 4 * 9 * C * K, D.pack_conv_w(d['W']).ravel())
        self.inputs.append(self.wp)
        b = R.bias_of(kind, d)
        self.bias = V(gpu, b.shape, view, b) if b is not None else None
        if self.bias is not None:
            self.inputs.append(self.bias)
        tr = kind == 'dgrad'
        self.w = None
        if kind != 'wgrad':
            if self.fam == 'f32':
                self.w = self.wp
                if tr:
                    self.w = Raw(gpu, 4 * 9 * C * K)
                    ops.transpose_weights(self.desc, self.wp.t, self.w.t)
            else:
                self.w = Raw(gpu, ops.lp_weight_bytes(self.desc, tr, mode))
                ops.lp_pack_weights(self.desc, self.wp.t, self.w.ptr, mode, tr)
            if self.w is not self.wp:
                self.w.snapshot()
                self.inputs.append(self.w)
        else:
            need = ops.wgrad_workspace(self.desc) if self.fam == 'f32' else ops.wgrad_lp_workspace(self.desc)
            self.ws = Raw(gpu, need)
            self.buffers.append(self.ws)
        self.xq = self.dyq = None
        if self.fam == 'split' and kind == 'wgrad':
            self.xq = self.pack(self.x, xs)
        if self.fam == 'split' and kind != 'fwd':
            self.dyq = self.pack(self.dy, ys)
        self.yact = None

    def pack(self, v, shape):
        q = QV(self.gpu, shape, self.mode, self.view)
        self.gpu[1].q_pack(v.t, q.q)
        q.snapshot()
        self.inputs.append(q)
        return q

    def out(self, prev=None):
        shape = R.out_shape(self.kind, self.g)
        if self.kind == 'wgrad':
            return Raw(self.gpu, 4 * int(np.prod(shape)), None if prev is None else self.gpu[2].pack_conv_w(prev).ravel())
        return V(self.gpu, shape, self.view, prev)

    def read(self, o):
        if self.kind == 'wgrad':
            N, C, H, W, K = self.g
            return self.gpu[2].unpack_conv_w(o.numpy(), K, C, 3, 3)
        return o.numpy()

    def call(self, o, act='linear', bias=False, accumulate=False):
        dev, ops, D = self.gpu
        d, m, b = self.desc, self.mode, (self.bias.t if bias else None)
        if self.kind == 'fwd':
            if self.fam == 'f32':
                ops.conv2d_fwd(d, self.x.t, self.w.t, b, o.t, act, R.SLOPE, accumulate)
            else:
                ops.conv2d_fwd_lp(d, self.x.t, self.w.ptr, b, o.t, m, act, R.SLOPE, accumulate)
        elif self.kind == 'dgrad':
            if self.fam == 'f32':
                ops.conv2d_dgrad_t(d, self.dy.t, self.w.t, o.t, b, act, R.SLOPE, accumulate)
            else:
                ops.conv2d_dgrad_lp(d, self.dy.t, self.w.ptr, o.t, m, b, act, R.SLOPE, accumulate)
        elif self.fam == 'f32':
            ops.conv2d_wgrad(d, self.x.t, self.dy.t, o.t, self.ws.ptr, accumulate)
        elif self.fam == 'lp':
            ops.conv2d_wgrad_lp(d, self.x.t, self.dy.t, o.t, self.ws.ptr, m, accumulate)
        else:
            ops.conv2d_wgrad_lp_q(d, self.xq.q, self.dyq.q, o.t, self.ws.ptr, m, accumulate)
        return self.read(o)

    def dact_form(self):
        if self.fam == 'split':         # (Ops.dgrad_dact_supported falls back to the fp32 form for a split plan in split-K form)
            return 3 if load().ghm_split_dgrad_dact_supported(C.byref(self.desc)) else 0
        return self.gpu[1].dgrad_dact_supported(self.desc, self.mode)

    def call_dact(self, o, act):
        dev, ops, D = self.gpu
        if self.yact is None:
            self.yact = V(self.gpu, R.out_shape('dgrad', self.g), self.view, self.d['yact'])
            self.inputs.append(self.yact)
        if self.fam == 'split':
            ops.conv2d_dgrad_dact_lp_q(self.desc, self.dyq.q, self.w.ptr, o.t, None, self.yact.t, act, R.SLOPE, self.mode)
        else:
            ops.conv2d_dgrad_dact(self.desc, self.dy.t, self.w.t if self.fam == 'f32' else self.w.ptr, o.t, self.yact.t, act,
                                  R.SLOPE, self.mode)
        return o.numpy()

    def settle(self, what, outs):
        unchanged(what, *self.inputs)
        clean(what, *(self.buffers + outs))
        for o in outs:
            self.gpu[0].free(o.base)


def refs(mode, kind, g, d, key):
    """(ref without bias, ref with bias, M with bias) of the row's real inputs, cached per geometry and reference class"""
    cls = {'f32': 'raw', 'bf16x3': 'raw'}.get(mode, mode)
    mcls = 'raw' if cls in ('raw', 'bf16x2') else cls

    def make():
        b = R.bias_of(kind, d)
        r0 = R.ref_mode(mode, kind, d['x'], d['W'], None, d['dy'])
        return r0, (r0 if b is None else r0 + np.asarray(b, np.float64)[None, :, None, None])
    r0, rb = cached((key, g, kind, cls), make)
    M = cached((key, g, kind, 'M', mcls), lambda: R.M(mode, kind, d['x'], d['W'], R.bias_of(kind, d), d['dy']))
    return r0, rb, M


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row(gpu, mem, row):
    mode, kind, g = row.mode, row.kind, row.g
    with tuning_env(**row.env):
        # ---- 1. integer pass ----
        di = cached(('int', g), lambda: R.int_inputs(g))
        iref = cached(('iref', g, kind), lambda: R.ref(kind, di['x'], di['W'], None, di['dy']))
        ib = R.bias_of(kind, di)
        irb = iref if ib is None else iref + ib.astype(np.float64)[None, :, None, None]
        p = Product(gpu, mode, kind, g, row.view, di)
        outs = [p.out()]
        exact((mode, kind), p.call(outs[-1]), iref, "integers, plain", at=kind)
        if kind != 'wgrad':
            for act in ('lrelu', 'relu'):
                outs.append(p.out())
                exact((mode, kind), p.call(outs[-1], act, bias=True), act64(irb, act), "integers, bias + %s" % act, at=kind, zero_sign=act != 'relu')
        outs.append(p.out(di['prev'][kind]))
        exact((mode, kind), p.call(outs[-1], accumulate=True), di['prev'][kind] + iref, "integers, accumulate", at=kind)
        if kind == 'dgrad':
            assert p.dact_form() == row.reaches['dact'], (p.dact_form(), row.reaches)
            if row.reaches['dact']:
                for act in ('lrelu', 'relu'):
                    outs.append(p.out())
                    exact((mode, kind), p.call_dact(outs[-1], act), iref * slope64(di['yact'], act), "integers, dact %s" % act, at=kind)
        p.settle((R.row_id(row), "integer pass"), outs)
        # ---- 2. real pass ----
        dr = cached(('real', g), lambda: R.real_inputs(g))
        r0, rb, M = refs(mode, kind, g, dr, 'real')
        p = Product(gpu, mode, kind, g, row.view, dr)
        o1, o2, o3 = p.out(), p.out(), p.out()
        got = p.call(o1, bias=kind != 'wgrad')
        note((mode, kind), got, rb, M, "real", at=kind)
        again = p.call(o2, bias=kind != 'wgrad')
        exact((mode, kind), again, got, "real, repeated call", at=kind)
        inc = p.call(o3) if kind != 'wgrad' else got
        o4 = p.out(dr['prev'][kind])
        acc = p.call(o4, accumulate=True)
        exact((mode, kind), acc, (dr['prev'][kind] + inc).astype(np.float32), "real, accumulate == fl32(previous + increment)", at=kind)
        outs = [o1, o2, o3, o4]
        if kind == 'dgrad' and row.reaches['dact']:
            outs.append(p.out())
            s = slope64(dr['yact'], 'lrelu')
            note((mode, kind), p.call_dact(outs[-1], 'lrelu'), r0 * s, (M - np.abs(dr['bc'].astype(np.float64))[None, :, None, None]) * s, "real, dact lrelu", at=kind)
        p.settle((R.row_id(row), "real pass"), outs)


@pytest.mark.parametrize("q", R.Q_ROWS, ids=lambda q: "%s-%s-%s" % (q[0], q[1], q[3]))
def test_q_operands(gpu, mem, q):
    """the q-output and q-input forms: q output == pieces(fp32 output of the same call), q-input call == fp32-input call"""
    mode, kind, g, view = q
    dev, ops, D = gpu
    dr = cached(('real', g), lambda: R.real_inputs(g))
    r0, rb, M = refs(mode, kind, g, dr, 'real')
    p = Product(gpu, mode, kind, g, 'whole', dr)
    assert ops.lp_q_direct(p.desc, R.KIND_CODE[kind], mode)
    src, sshape = (p.x, R.shapes(g)[0]) if kind == 'fwd' else (p.dy, R.shapes(g)[2])
    inq = QV(gpu, sshape, mode, view)           # the q input in the row's view spec
    ops.q_pack(src.t, inq.q)
    inq.snapshot()
    p.inputs.append(inq)
    for want, have in zip(R.pieces(src.data, mode), inq.pieces()):
        assert Q.bits_equal(have, want)
    o1, o2 = p.out(), p.out()
    y1 = p.call(o1, 'lrelu', bias=True)
    note((mode, kind), y1, act64(rb, 'lrelu'), M, "q row, fp32 input", at=kind)
    outq = QV(gpu, R.out_shape(kind, g), mode, view)
    if kind == 'fwd':
        ops.conv2d_fwd_lp_q(p.desc, inq.q, p.w.ptr, p.bias.t, o2.t, outq.q, mode, 'lrelu', R.SLOPE)
    else:
        ops.conv2d_dgrad_lp_q(p.desc, inq.q, p.w.ptr, o2.t, outq.q, mode, p.bias.t, 'lrelu', R.SLOPE)
    y2 = o2.numpy()
    exact((mode, kind), y2, y1, "q input == fp32 input", at=kind)
    for i, (want, have) in enumerate(zip(R.pieces(y2, mode), outq.pieces())):
        exact((mode, kind), have, want, "q output piece %d == pieces(fp32 output)" % i, at=kind)
    only = QV(gpu, R.out_shape(kind, g), mode, view)          # the fp32 pointer NULL: the q result is unchanged
    if kind == 'fwd':
        ops.conv2d_fwd_lp_q(p.desc, inq.q, p.w.ptr, p.bias.t, None, only.q, mode, 'lrelu', R.SLOPE)
    else:
        ops.conv2d_dgrad_lp_q(p.desc, inq.q, p.w.ptr, None, only.q, mode, p.bias.t, 'lrelu', R.SLOPE)
    for want, have in zip(outq.pieces(), only.pieces()):
        assert Q.bits_equal(have, want)
    clean((q, "q outputs"), outq, only)
    p.settle((q, "q row"), [o1, o2])
