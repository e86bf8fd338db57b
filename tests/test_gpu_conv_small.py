"""The small-map convolutions of csrc/conv_small.hip (sm_gemm_kernel in its nine (NTAPS, NQ) instantiations, sm_finish_kernel
in both forms with and without the BatchNorm, sm_q_pack_kernel) through device.Ops in 'bf16' and 'f16', per element and inside
canary views, at the rows of tests/conv_small_ref.py (each row names the variant, parity classes, image group, split count,
slabs per block and ring depth it reaches; tests/test_conv_small_ref.py checks those claims against ghm_sm_plan_query, the
inputs and every bound on the CPU).

Per row, under the row's tuning environment (entered once per row):
  1. integer pass: inputs of small integers (any summation order exact, every operand exact in bf16 and fp16) -- the fp32
     output equals the float64 answer BIT FOR BIT: linear, leaky relu 0.25 and relu, each with and without bias, and
     accumulating onto integers; the q output equals round(fp32 output) bit for bit and is the same with the fp32 output
     omitted; the fp32-operand entry (sm_q_pack_kernel reading a channel slice of a wider buffer) gives the bits of the
     q-operand entry;
  2. real pass: |got - ref| <= k 2^-24 M per element (k, M: tests/conv_small_ref.py) and the rel-L2 bound of the older tests;
     a failure names the element and its border / parity class; a repeated call gives identical bits; accumulate is exactly
     fl32(previous + finished sum) (sm_finish_kernel's ``v += *o`` after the bias and every partial);
  3. nothing else is written and nothing outside a view is read: the q operand, the q output and the fp32 output live in the
     row's view (whole / channel slice of a wider buffer / offset start) inside NaN-canary allocations, the fp32 operand in a
     channel slice, the weight pack (exactly ghm_lp_weight_bytes long) and the bias in exact-size buffers between 4 KB guards;
     no canary changes, the inputs are bit-unchanged, the outputs are finite, and the bits are the same after everything
     outside the views is repainted with a finite pattern.
For a fixed split count every ring depth gives identical bits (the partial sums do not depend on the ring).  The BatchNorm rows
hold conv_out per element as above, y / mean / inv / running statistics per element against the float64 BatchNorm of the
kernel's own conv_out, the q output to round(y), the all-zero filter's channel to mean == bias, inv == fl32(1 / sqrt(eps)),
y == act(beta) bit for bit, and the running statistics untouched when none are passed -- through sm_conv, through
lp_conv_kernel's split-K partials and through the fp32 ghm_conv2d_bn_fwd.  The plan that runs is the plan the host-only query
reports: sm_conv plans with the queries' CU count (asserted equal to the device's on the MI355X).

Measured on the MI355X (the module prints this table when it finishes): max over all rows and calls of |got - ref| / (2^-24 M)
against the asserted k, the largest rel-L2 (bound 2e-5 against the rounded operands), the number of comparisons (bit-exact ones
included):
  bf16  forward         1.84 of 11   1.5e-07  (821)        BatchNorm y           2.87 of 7   1.5e-07  (94)
  bf16  data gradient   1.85 of  8   1.7e-07  (605)        batch mean            0.98 of 2   3.8e-08  (38)
  f16   forward         1.96 of 17   1.6e-07  (821)        inverse std           0.98 of 2   1.3e-08  (38)
  f16   data gradient   2.66 of 12   1.8e-07  (605)        running statistics    1.81 of 4   6.6e-08  (57)
  f32   conv_out of ghm_conv2d_bn_fwd   3.81 of 7   1.9e-07  (4)
Every integer comparison was bit-exact in every variant, class pattern, split count and ring depth (3 .. 8, blocks of up to 32
slabs), every ring depth gave the bits of the shallowest, every accumulate was exactly fl32(previous + finished sum), every
repeated call bit-identical, the all-zero filter's channel came out as stated, no canary changed and no result depended on
bytes outside a view: no kernel needed a fix.  The first run failed on one mistake of the module's own (it expected three
distinct ring depths from a group whose budgets give two).  Wall time on the MI355X: 155 tests in 1.7 - 2.4 s (1.0 - 1.6 s between the
fixture's start and end).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import GhmError, call, tuning_env
from oracle import lp as LP
from tests import canary
from tests import conv_small_ref as R
from tests import elementwise_q_ref as Q

pytestmark = pytest.mark.gpu

BOUND = dict(R.K_BOUND, bn=R.K_BN, mean=R.K_MEAN, inv=R.K_INV, run=R.K_RUN)
_REF = {}
LEDGER = canary.Ledger(lambda key, w, r, n: "measured %-16s worst k %7.3f of %2d  rel-L2 %.2e  (%d comparisons)"
                       % (" ".join(key) if isinstance(key, tuple) else key, w, BOUND[key], r, n),
                       bound=BOUND.__getitem__, rel_limit=None, order=lambda m: sorted(m, key=str), header="",
                       describe=lambda at, i, shape: R.element_class(at[0], at[1], i) if len(shape) == 4 else "channel")
gpu, mem = canary.fixtures(LEDGER, _REF)
cached = functools.partial(canary.cached, _REF)
V, Buf, QV = canary.View.named, canary.Bytes, canary.QView.named
clean, unchanged, repaint, note, exact = canary.clean, canary.unchanged, canary.repaint, LEDGER.note, LEDGER.exact


def vec(gpu, a):
    """a per-channel vector in an exact-size buffer between two canary guards"""
    return Buf(gpu, 4 * len(a), np.asarray(a, np.float32))


def plan_query(D, desc, kind, mode):
    out = (C.c_int32 * 12)()
    call("ghm_sm_plan_query", C.byref(desc), R.KIND_CODE[kind], D.DTYPE_CODES[mode], C.byref(out))
    return list(out)


class Product:
    """the operands of one row on the device, and its calls"""

    def __init__(self, gpu, mode, kind, g, view, d):
        self.gpu, self.mode, self.kind, self.g, self.view = gpu, mode, kind, g, view
        dev, ops, D = gpu
        N, Cc, H, W, K, k, s, pad = g
        src = d['x'] if kind == 'fwd' else d['dy']
        self.src = V(gpu, R.in_shape(kind, g), 'slice', src)           # the fp32 operand: a channel slice of a wider buffer
        self.out_ns = R.view_layout(R.out_shape(kind, g), view)[1]
        xns, yns = (self.src.t.nstride, self.out_ns) if kind == 'fwd' else (self.out_ns, self.src.t.nstride)
        self.desc = D.conv_desc(N, Cc, H, W, K, k, k, s, pad, xns, yns)
        self.inq = QV(gpu, R.in_shape(kind, g), mode, view)
        ops.q_pack(self.src.t, self.inq.q)
        self.inq.snapshot()
        assert Q.bits_equal(self.inq.pieces()[0], LP.ROUND[mode](src))
        tr = kind == 'dgrad'
        wp = Buf(gpu, 4 * k * k * Cc * K, D.pack_conv_w(d['W']))
        self.wq = Buf(gpu, ops.lp_weight_bytes(self.desc, tr, mode))       # exactly the documented size
        ops.lp_pack_weights(self.desc, wp.ptr, self.wq.ptr, mode, tr)
        self.wq.data = self.wq.bytes()
        self.bias = vec(gpu, R.bias_of(kind, d))
        self.inputs = [self.src, self.inq, wp, self.wq, self.bias]
        self.outs = []

    def out(self, prev=None):
        o = V(self.gpu, R.out_shape(self.kind, self.g), self.view, prev)
        self.outs.append(o)
        return o

    def outq(self):
        o = QV(self.gpu, R.out_shape(self.kind, self.g), self.mode, self.view)
        self.outs.append(o)
        return o

    def call(self, o, oq=None, act='linear', bias=False, accumulate=False, fp32_operand=False):
        dev, ops, D = self.gpu
        d, m, b = self.desc, self.mode, (self.bias.ptr if bias else None)
        ot, oqt = (o.t if o is not None else None), (oq.q if oq is not None else None)
        if fp32_operand:
            if self.kind == 'fwd':
                ops.conv2d_fwd_lp(d, self.src.t, self.wq.ptr, b, ot, m, act, R.SLOPE, accumulate)
            else:
                ops.conv2d_dgrad_lp(d, self.src.t, self.wq.ptr, ot, m, b, act, R.SLOPE, accumulate)
        elif self.kind == 'fwd':
            ops.conv2d_fwd_lp_q(d, self.inq.q, self.wq.ptr, b, ot, oqt, m, act, R.SLOPE, accumulate)
        else:
            ops.conv2d_dgrad_lp_q(d, self.inq.q, self.wq.ptr, ot, oqt, m, b, act, R.SLOPE, accumulate)
        return o.numpy() if o is not None else None

    def everything(self):
        return self.inputs + self.outs

    def settle(self, what):
        unchanged(what, *self.inputs)
        clean(what, *self.outs)
        for o in self.outs:
            self.gpu[0].free(o.ptr)
        self.outs = []


def with_bias(ref, b):
    return ref + np.asarray(b, np.float64)[None, :, None, None]


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row(gpu, mem, row):
    mode, kind, g, key = row.mode, row.kind, row.g, (row.mode, row.kind)
    dev, ops, D = gpu
    rnd = LP.ROUND[mode]
    with tuning_env(**row.env):
        # ---- 1. integer pass ----
        di = cached(('int', g), lambda: R.int_inputs(g))
        iref = cached(('iref', g, kind), lambda: R.ref(kind, g, di['x'], di['W'], None, di['dy']))
        irb = with_bias(iref, R.bias_of(kind, di))
        p = Product(gpu, mode, kind, g, row.view, di)
        # the plan that runs is the plan the query reports, and the row's claim
        q = plan_query(D, p.desc, kind, mode)
        assert q[0] == 1 and (q[2], q[3], tuple((q[11] >> (8 * c)) & 255 for c in range(q[1]))) + tuple(q[4:9]) == row.reaches, q
        assert dev.info()['num_cu'] == R.CUS, dev.info()
        for act in ('linear', 'lrelu', 'relu'):
            for bias in (False, True):
                o, oq = p.out(), p.outq()
                want = R.act64(irb if bias else iref, act)
                what = "integers, %s%s" % ("bias + " if bias else "", act)
                exact(key, p.call(o, oq, act, bias=bias), want, what, at=(kind, g), zero_sign=act != 'relu')
                exact(key, oq.pieces()[0], rnd(want), what + ": q output == round(fp32 output)", at=(kind, g), zero_sign=act != 'relu')
                if act == 'lrelu' and bias:
                    only = p.outq()
                    p.call(None, only, act, bias=True)
                    assert np.array_equal(only.raw()[only.inside], oq.raw()[oq.inside]), "the q output changes when the fp32 output is omitted"
                    exact(key, p.call(p.out(), None, act, bias=True, fp32_operand=True), want, what + ", fp32 operand", at=(kind, g))
        o, oq = p.out(di['prev'][kind]), p.outq()
        acc = di['prev'][kind] + irb
        exact(key, p.call(o, oq, bias=True, accumulate=True), acc, "integers, accumulate", at=(kind, g))
        exact(key, oq.pieces()[0], rnd(acc), "integers, accumulate: q output", at=(kind, g))
        p.settle((R.row_id(row), "integer pass"))
        # ---- 2. real pass ----
        dr = cached(('real', g), lambda: R.real_inputs(g))
        b = R.bias_of(kind, dr)
        ref = cached(('ref', g, kind, mode), lambda: R.ref_mode(mode, kind, g, dr['x'], dr['W'], b, dr['dy']))
        M = cached(('M', g, kind, mode), lambda: R.M(mode, kind, g, dr['x'], dr['W'], b, dr['dy']))
        p = Product(gpu, mode, kind, g, row.view, dr)
        o1, q1 = p.out(), p.outq()
        got = p.call(o1, q1, bias=True)
        note(key, got, ref, M, "real", at=(kind, g), rel_limit=R.REL_L2[mode])
        exact(key, q1.pieces()[0], rnd(got), "real: q output == round(fp32 output)", at=(kind, g))
        o2, q2 = p.out(), p.outq()
        exact(key, p.call(o2, q2, bias=True), got, "real, repeated call", at=(kind, g))
        assert np.array_equal(q2.raw()[q2.inside], q1.raw()[q1.inside])
        exact(key, p.call(p.out(), None, bias=True, fp32_operand=True), got, "real, fp32 operand == q operand", at=(kind, g))
        o4 = p.out(dr['prev'][kind])
        exact(key, p.call(o4, None, bias=True, accumulate=True), (dr['prev'][kind] + got).astype(np.float32), "real, accumulate == fl32(previous + finished sum)", at=(kind, g))
        unchanged((R.row_id(row), "real pass"), *p.inputs)
        clean((R.row_id(row), "real pass"), *p.outs)
        # ---- 3. nothing outside the views is read: the same bits over a finite pattern ----
        o5, q5 = p.out(), p.outq()
        repaint(dev, *p.everything())
        exact(key, p.call(o5, q5, bias=True), got, "real, everything outside the views repainted", at=(kind, g))
        assert np.array_equal(q5.raw()[q5.inside], q1.raw()[q1.inside])
        exact(key, p.call(p.out(), None, bias=True, fp32_operand=True), got, "real, repainted, fp32 operand", at=(kind, g))


RING_GROUPS = [(kind, g, [dict(R.SPLIT1, GHM_SM_LDS_KB=str(kb)) for kb in R.RING_KB]) for kind, g in R.RING_SHAPES] + \
              [('dgrad', R.DEEP, [dict(R.SPLIT1, GHM_SM_LDS_KB=str(kb)) for kb, _ in R.DEEP_KB])]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("group", RING_GROUPS, ids=lambda t: "%s-%s" % (t[0], "x".join(str(v) for v in t[1])))
def test_every_ring_depth_gives_the_same_bits(gpu, mem, group, mode):
    """one split: the partial sums do not depend on the ring depth"""
    kind, g, envs = group
    dev, ops, D = gpu
    dr = cached(('real', g), lambda: R.real_inputs(g))
    p = Product(gpu, mode, kind, g, 'whole', dr)
    first, depths = None, set()
    for env in envs:
        with tuning_env(**env):
            depths.add(plan_query(D, p.desc, kind, mode)[8])
            got = p.call(p.out(), None, bias=True)
        if first is None:
            first = got
        exact((mode, kind), got, first, "ring budget %s KB against %s KB" % (env['GHM_SM_LDS_KB'], envs[0]['GHM_SM_LDS_KB']), at=(kind, g))
    assert len(depths) >= 2, depths
    p.settle((group[:2], mode, "ring depths"))


BN_CASES = [(row, mode) for row in R.BN_ROWS for mode in (R.MODES if row.path != 'f32' else ('f32',))]


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%s-%s" % (R.bn_row_id(c[0]), c[1]))
def test_batchnorm_row(gpu, mem, case):
    row, mode = case
    dev, ops, D = gpu
    g = row.g
    N, Cc, H, W, K, k, s, pad = g
    rnd, z, key = LP.ROUND[mode], R.ZERO_CHANNEL, (mode, 'fwd')
    d = cached(('bn', g), lambda: R.bn_inputs(g))
    ys = R.out_shape('fwd', g)
    yv, qv = ('slice', 'offset') if R.BN_ROWS.index(row) % 2 == 0 else ('offset', 'slice')       # the views of y and of the q output
    with tuning_env(**row.env):
        x = V(gpu, R.in_shape('fwd', g), 'slice', d['x'])
        co_ns = R.view_layout(ys, 'slice')[1]
        desc = D.conv_desc(N, Cc, H, W, K, k, k, s, pad, x.t.nstride, co_ns)
        wp = Buf(gpu, 4 * k * k * Cc * K, D.pack_conv_w(d['W']))
        inputs = [x, wp]
        if mode != 'f32':
            xq = QV(gpu, R.in_shape('fwd', g), mode, 'slice')
            ops.q_pack(x.t, xq.q)
            xq.snapshot()
            wq = Buf(gpu, ops.lp_weight_bytes(desc, False, mode))
            ops.lp_pack_weights(desc, wp.ptr, wq.ptr, mode, False)
            wq.data = wq.bytes()
            inputs += [xq, wq]
            assert ops.conv_bn_fused_supported(desc, mode) and bool(plan_query(D, desc, 'fwd', mode)[0]) == (row.path == 'sm')
        vecs = dict(b=vec(gpu, d['b']), gamma=vec(gpu, d['gamma']), beta=vec(gpu, d['beta']))
        inputs += list(vecs.values())
        ref = cached(('bnref', g, mode), lambda: R.ref_mode(mode, 'fwd', g, d['x'], d['W'], d['b'], None))
        M = cached(('bnM', g, mode), lambda: R.M(mode, 'fwd', g, d['x'], d['W'], d['b'], None))

        def run(act, running, want_y=True, want_q=True):
            o = dict(co=V(gpu, ys, 'slice'), y=V(gpu, ys, yv) if want_y else None,
                     yq=QV(gpu, ys, mode, qv) if want_q and mode != 'f32' else None,
                     mean=Buf(gpu, 4 * K), inv=Buf(gpu, 4 * K), rm=vec(gpu, d['rm']), ri=vec(gpu, d['ri']))
            rm, ri = (o['rm'].ptr, o['ri'].ptr) if running else (None, None)
            if mode == 'f32':
                ops.conv2d_bn_fwd(desc, x.t, wp.ptr, vecs['b'].ptr, o['co'].t, o['y'].t, vecs['gamma'].ptr, vecs['beta'].ptr,
                                  o['mean'].ptr, o['inv'].ptr, rm, ri, R.BN_EPS, R.BN_ALPHA, act, R.BN_SLOPE)
            else:
                ops.conv2d_bn_fwd_lp_q(desc, xq.q, wq.ptr, vecs['b'].ptr, o['co'].t, o['y'].t if want_y else None,
                                       o['yq'].q if o['yq'] is not None else None, vecs['gamma'].ptr, vecs['beta'].ptr, o['mean'].ptr,
                                       o['inv'].ptr, rm, ri, R.BN_EPS, R.BN_ALPHA, mode, act, R.BN_SLOPE)
            return o

        o = run('lrelu', True)
        t = o['co'].numpy()
        note(key, t, ref, M, "BatchNorm row: conv_out", at=('fwd', g), rel_limit=R.REL_L2.get(mode, 1e-5))
        exact(key, t[:, z], np.broadcast_to(d['b'][z], t[:, z].shape), "conv_out of the all-zero filter == bias", at=('fwd', g))
        want = R.bn_ref(t, d, 'lrelu', R.BN_SLOPE)
        y, mean, inv = o['y'].numpy(), o['mean'].numpy(), o['inv'].numpy()
        note('bn', y, want['y'], want['M'], "y", at=('fwd', g))
        note('mean', mean, want['mean'], want['M_mean'], "mean", at=('fwd', g))
        note('inv', inv, want['inv'], want['inv'], "inv", at=('fwd', g))
        note('run', o['rm'].numpy(), want['rm'], want['M_rm'], "running mean", at=('fwd', g))
        note('run', o['ri'].numpy(), want['ri'], want['M_ri'], "running inverse std", at=('fwd', g))
        if o['yq'] is not None:
            exact('bn', o['yq'].pieces()[0], rnd(y), "q output == round(y)", at=('fwd', g))
        # the all-zero filter: zero variance (the var < 0 clamp's neighbourhood)
        assert mean[z] == d['b'][z] and inv[z] == np.float32(1.0 / np.sqrt(float(np.float32(R.BN_EPS)))), (mean[z], inv[z])
        beta_z = np.float32(d['beta'][z])
        exact('bn', y[:, z], np.broadcast_to(beta_z if beta_z > 0 else np.float32(R.BN_SLOPE) * beta_z, y[:, z].shape), "y of the all-zero filter == act(beta)", at=('fwd', g))
        outs = [v for v in o.values() if v is not None]
        unchanged((R.bn_row_id(row), mode), *inputs)
        clean((R.bn_row_id(row), mode), *outs)
        # no running statistics passed: theirs stay as they were; the q output alone; linear
        o2 = run('lrelu', False, want_y=mode == 'f32')
        assert o2['rm'].same() and o2['ri'].same(), "running statistics written without being passed"
        exact(key, o2['co'].numpy(), t, "repeated call: conv_out", at=('fwd', g))
        exact('mean', o2['mean'].numpy(), mean, "repeated call: mean", at=('fwd', g))
        exact('inv', o2['inv'].numpy(), inv, "repeated call: inv", at=('fwd', g))
        if o2['yq'] is not None:
            assert np.array_equal(o2['yq'].raw()[o2['yq'].inside], o['yq'].raw()[o['yq'].inside]), "the q output changes without y"
        o3 = run('linear', True, want_q=False)
        note('bn', o3['y'].numpy(), R.bn_ref(t, d, 'linear')['y'], want['M'], "y, linear", at=('fwd', g))
        outs += [v for oo in (o2, o3) for v in oo.values() if v is not None]
        clean((R.bn_row_id(row), mode, "second and third call"), *outs)
        # nothing outside the views is read
        repaint(dev, *(inputs + outs))
        o4 = run('lrelu', True)
        exact('bn', o4['y'].numpy(), y, "everything outside the views repainted: y", at=('fwd', g))
        exact(key, o4['co'].numpy(), t, "repainted: conv_out", at=('fwd', g))
        exact('run', o4['rm'].numpy(), o['rm'].numpy(), "repainted: running mean", at=('fwd', g))
        clean((R.bn_row_id(row), mode, "repainted"), *[v for v in o4.values() if v is not None])


@pytest.mark.parametrize("mode", R.MODES)
def test_refusals_write_nothing(gpu, mem, mode):
    """an unserved geometry (6 x 6 map, 16 filters: neither the small-map nor the split-K form) and a q tensor off 16-byte
    alignment through conv2d_bn_fwd_lp_q are errors before anything is launched"""
    dev, ops, D = gpu
    for g, shift in (((2, 16, 6, 6, 16, 3, 1, 1), 0), ((3, 16, 4, 4, 16, 3, 1, 1), 8)):
        N, Cc, H, W, K, k, s, pad = g
        d = R.bn_inputs(g)
        desc = D.conv_desc(N, Cc, H, W, K, k, k, s, pad)
        assert bool(ops.conv_bn_fused_supported(desc, mode)) == (shift != 0)
        x = V(gpu, R.in_shape('fwd', g), 'whole', d['x'])
        xq = QV(gpu, R.in_shape('fwd', g), mode, 'whole')
        ops.q_pack(x.t, xq.q)
        xq.snapshot()
        wq = Buf(gpu, ops.lp_weight_bytes(desc, False, mode))
        ops.lp_pack_weights(desc, Buf(gpu, 4 * k * k * Cc * K, D.pack_conv_w(d['W'])).ptr, wq.ptr, mode, False)
        wq.data = wq.bytes()
        vs = [vec(gpu, d[n]) for n in ('b', 'gamma', 'beta', 'rm', 'ri')]
        ys = R.out_shape('fwd', g)
        outs = [Buf(gpu, 4 * int(np.prod(ys))), Buf(gpu, 4 * int(np.prod(ys))), Buf(gpu, 2 * int(np.prod(ys))), Buf(gpu, 4 * K), Buf(gpu, 4 * K)]
        bad = D.QTensor(dev, xq.q.ptr + shift, xq.q.shape, mode)
        with pytest.raises(GhmError):
            ops.conv2d_bn_fwd_lp_q(desc, bad, wq.ptr, vs[0].ptr, outs[0].tensor(ys), outs[1].tensor(ys),
                                   D.QTensor(dev, outs[2].ptr, ys, mode), vs[1].ptr, vs[2].ptr, outs[3].ptr, outs[4].ptr, vs[3].ptr,
                                   vs[4].ptr, R.BN_EPS, R.BN_ALPHA, mode, 'lrelu', R.BN_SLOPE)
        dev.sync()
        for o in outs:
            assert o.untouched() and o.stray().size == 0, "a refused call wrote"
        unchanged((g, "refused"), xq, wq)
        for v in vs:
            assert v.same() and v.stray().size == 0
