"""The thin first- and last-layer convolutions of csrc/conv_thin.hip (fanout_kernel, fanin_s1_kernel, fanin_s2_kernel,
thin_wgrad_kernel and the pooled fan-out) through device.Ops, per element and inside canary views, at the rows of
tests/conv_thin_ref.py (each row names the instantiation and plan it reaches; tests/test_conv_thin_ref.py checks those claims,
the inputs and the bound on the CPU).

Per row, under the row's tuning environment, with x, dy, y, dx, the bias and the accumulate target in views (whole / channel
slice of a wider buffer / 80 bytes in) inside NaN-canary allocations, packed and transposed weights, dW, the mask and the
workspace as whole buffers with a canary head and tail:
  1. integer pass: the result equals the float64 answer BIT FOR BIT: plain, bias + leaky relu 0.25, bias + relu (there a zero
     of either sign), accumulating onto a known integer tensor; the pooled rows: the pooled values and every mask byte (bit
     2 dr + dc, all ties set, 16 where the maximum is positive), with tied windows present;
  2. real pass: |got - ref| <= k 2^-24 M per element and rel-L2 <= 1e-5; a repeated call is bit-identical; accumulate is exactly
     fl32(previous + increment), the increment being what the same call writes without accumulate (fanout ``vals += old``,
     fanin_s1 ``v += *o``, fanin_s2 ``r += old`` and ghm_reduce_splits all finish their sum and bias first -- read in the
     source); the kernel agrees with the general kernel it replaces (GHM_NO_THIN=1) inside 2 k; the pooled rows equal the
     unpooled fan-out forward pooled on the host, bit for bit, mask included; g_out's tanh (fanin_s1's ghm_act) is held to
     float64 tanh of the kernel's own linear output inside K_LIBM['in_fwd_tanh'] = 6 units of max(|tanh|, 2^-126).
     (Accumulate with a non-linear activation is refused by every entry point -- "accumulate needs a linear epilogue" -- so
     that form of the issue has nothing to run.)
  3. no canary changed, the inputs are bit-unchanged, the outputs are finite: what lies outside a view is NaN, so a read across
     an image border shows;
  4. persistent blocks: the rows of conv_thin_ref.MULTI run more than two (one) iterations per block on this device's CU count
     (asserted from ghm_device_info);
  5. q epilogue (conv2d_fwd_thin_q at KSTEPS 5, 13, 18; conv2d_fwd_pool_thin_q on the rows thin_fanout_fwd_pool serves, under
     GHM_NO_THIN_LP=1: thin_pool_lp of conv_thin_lp.hip is out of scope) in bf16, f16, bf16x3, bf16x2: every plane equals
     pieces(fp32 output of the same call), the q-only call gives the same planes, canaries round a 'slice' and an 'offset' q view;
  6. the alignment guard: an output view 4 bytes in is served by the general kernel (bit-identical to the GHM_NO_THIN=1 run) and
     comes out right, with clean canaries; the pooled entry point, which has no other kernel for <= 4 channels, refuses it and writes nothing.

Measured on the MI355X (the module prints this when it finishes): the worst |got - ref| / (2^-24 M) over all rows and calls
against the asserted k, the worst rel-L2 (bound 1e-5) and the number of comparisons (bit-exact ones included):
  fanout      fwd (+ pooled)   5.157 of  8   1.09e-07   (289)
  fanout      dgrad, dgrad_t   4.669 of  5   3.31e-08    (64)
  fanin_s1    fwd              1.558 of 12   1.97e-07    (32)
  fanin_s1    dgrad            1.740 of 13   2.49e-07    (24)
  fanin_s2    dgrad            6.870 of 11   4.67e-07    (48)
  thin_wgrad  wgrad            0.090 of  2   1.70e-07    (48)
  tanh (g_out): 2.288 of 6 units of max(|tanh|, 2^-126): the device-libm bound of tests/elementwise_f32_ref.py transfers.
No asserted k exceeds n + S + 2 (the smallest n is 9: the 3x3 one-channel forward).  Every integer comparison was bit-exact in
every instantiation, plan and view, the rows with two and three iterations per persistent block included; every mask byte
matched; every accumulate was exactly fl32(previous + increment); every repeated call was bit-identical; every q plane equalled
pieces(fp32 output); no canary changed and no result depended on bytes outside an input view: no kernel of conv_thin.hip needed
a fix.  Wall time on the MI355X: 105 tests in 23.0 s (22.2 s between the fixture's start and end).

One check exposed a weakness outside conv_thin.hip, and it is fixed: test_row_agrees_with_the_general_kernel found
fanout_kernel<dgrad> and the general kernel 12.91 x 2^-24 M apart on the 5x64x104x128 row, against 2 k = 10.  The thin kernel
stood 4.03 units from the float64 reference, the general one 12.52 (9.17, 9.32 and 6.63 on the other 'dgrad' rows):
smallk1_dgrad_kernel and smallk_dgrad_kernel (csrc/conv_igemm.hip) started their fmaf chain AT the bias, so every one of the
25 steps rounded at the magnitude of bias + partial sum.  A numpy restatement of that chain reproduced the 12.52 to the digit,
and 4.03 with the bias added after the products.  Both kernels now add it last (bit-identical to each other as before, and
bit-identical to their former selves where no bias is given, which is every data gradient of the train step); the general
kernel then stands 4.03, 4.07, 3.76 and 2.65 units from the reference and, for one filter, returns the thin kernel's very
bits, as igemm_kernel on one input channel does for the forward.  Library changes: that, and the alignment guard of the three
fan-out predicates.
"""
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import GhmError, tuning_env
from tests import canary
from tests import conv_thin_ref as R
from tests import elementwise_q_ref as Q
from tests.elementwise_f32_ref import K_LIBM

pytestmark = pytest.mark.gpu

TANH = [0.0]
_REF = {}
LEDGER = canary.Ledger(lambda key, w, r, n: "measured %-10s %-6s worst k %7.3f of %2d  rel-L2 %.2e  (%d comparisons)" % (key + (w, R.K_BOUND[key], r, n)),
                       bound=R.K_BOUND.__getitem__, rel_limit=R.REL_L2, describe=lambda at, i, shape: R.border_class(at[0], at[1], i),
                       footer=lambda: "tanh: worst %.3f of %d units of max(|tanh|, 2^-126)" % (TANH[0], K_LIBM['in_fwd_tanh']))
gpu, mem = canary.fixtures(LEDGER, _REF)
# the float64 references per geometry, shared by the rows that follow each other; the oldest leave (they are 16 - 70 MB)
cached = functools.partial(canary.cached, _REF, keep=10)
V, Raw, QV = canary.View.named, canary.Bytes.rounded, canary.QView.named
clean, unchanged, note, exact = canary.clean, canary.unchanged, LEDGER.note, LEDGER.exact


class Product:
    """the operands of one row on the device, and its calls"""

    def __init__(self, gpu, kind, g, view, d, out_view=None):
        self.gpu, self.kind, self.g, self.view, self.d = gpu, kind, g, view, d
        self.out_view = out_view or (view if kind != 'pool' or view != 'slice' else 'whole')      # (the pooled output is dense)
        dev, ops, D = gpu
        N, C, H, W, K, k, s, pad = g
        xs, ws, ys = R.shapes(g)
        base = R.base_kind(kind)
        self.x = V(gpu, xs, view, d['x']) if base != 'dgrad' else None
        self.dy = V(gpu, ys, view, d['dy']) if base != 'fwd' else None
        xns = self.x.t.nstride if self.x else R.view_layout(xs, self.out_view)[1]
        yns = self.dy.t.nstride if self.dy else R.view_layout(ys, self.out_view)[1]
        self.desc = D.conv_desc(N, C, H, W, K, k, k, s, pad, xns, yns)
        self.inputs = [v for v in (self.x, self.dy) if v is not None]
        self.buffers = []
        b = R.bias_of(kind, d)
        self.bias = V(gpu, b.shape, view, b) if b is not None else None
        if base != 'wgrad':
            self.w = Raw(gpu, 4 * k * k * C * K, D.pack_conv_w(d['W']).ravel())
            self.inputs += [self.w, self.bias]
            if kind == 'dgrad_t':
                self.wT = Raw(gpu, 4 * k * k * C * K)
                ops.transpose_weights(self.desc, self.w.t, self.wT.t)
                self.wT.snapshot()
                self.inputs.append(self.wT)
        else:
            self.ws = Raw(gpu, ops.wgrad_workspace(self.desc))
            self.buffers.append(self.ws)

    def out(self, prev=None):
        shape = R.out_shape(self.kind, self.g)
        if self.kind == 'wgrad':
            return Raw(self.gpu, 4 * int(np.prod(shape)), None if prev is None else self.gpu[2].pack_conv_w(prev).ravel())
        return V(self.gpu, shape, self.out_view, prev)

    def call(self, o, act='linear', bias=False, accumulate=False):
        dev, ops, D = self.gpu
        d, b = self.desc, (self.bias.t if bias else None)
        if self.kind == 'fwd':
            ops.conv2d_fwd(d, self.x.t, self.w.t, b, o.t, act, R.SLOPE, accumulate)
        elif self.kind == 'dgrad':
            ops.conv2d_dgrad(d, self.dy.t, self.w.t, o.t, b, act, R.SLOPE, accumulate)
        elif self.kind == 'dgrad_t':
            ops.conv2d_dgrad_t(d, self.dy.t, self.wT.t, o.t, b, act, R.SLOPE, accumulate)
        else:
            assert self.kind == 'wgrad'
            ops.conv2d_wgrad(d, self.x.t, self.dy.t, o.t, self.ws.ptr, accumulate)
            N, C, H, W, K, k, s, pad = self.g
            return D.unpack_conv_w(o.numpy(), K, C, k, k)
        return o.numpy()

    def call_pool(self, o, mask, act):
        dev, ops, D = self.gpu
        ops.conv2d_fwd_pool(self.desc, self.x.t, self.w.t, self.bias.t, o.t, mask.ptr, act, R.SLOPE, 'f32')
        return o.numpy(), self.mask_bytes(mask)

    def mask(self):
        return Raw(self.gpu, int(np.prod(R.out_shape('pool', self.g))))

    def mask_bytes(self, mask):
        shape = R.out_shape('pool', self.g)
        out = np.empty(int(np.prod(shape)), np.uint8)
        self.gpu[0].d2h(out, mask.ptr, out.nbytes)
        return out.reshape(shape)

    def settle(self, what, outs):
        unchanged(what, *self.inputs)
        clean(what, *(self.buffers + outs))
        for o in outs:
            self.gpu[0].free(o.base)


def refs(kind, g, d, key):
    """(ref without bias, ref with bias, M with bias) of a row's inputs, cached per geometry"""
    base = R.base_kind(kind)
    b = R.bias_of(kind, d)
    r0 = cached((key, g, base), lambda: R.ref(base, g, d['x'], d['W'], None, d['dy']))
    if key == 'int':
        return r0, (r0 if b is None else r0 + b.astype(np.float64)[None, :, None, None]), None
    m0 = cached((key, g, base, 'M'), lambda: R.M(base, g, d['x'], d['W'], None, d['dy']))
    if b is None:
        return r0, r0, m0
    return r0, r0 + b.astype(np.float64)[None, :, None, None], m0 + np.abs(b.astype(np.float64))[None, :, None, None]


def check_iterations(gpu, row):
    """a row that claims several iterations per persistent block must have them on THIS device"""
    if R.multi_key(row) in R.MULTI:
        cus = gpu[0].info()['num_cu']
        assert R.iterations(row) > R.MULTI[R.multi_key(row)] * cus, (R.row_id(row), R.iterations(row), cus)


@pytest.mark.parametrize("row", [r for r in R.ROWS if r.kind != 'pool'], ids=R.row_id)
def test_row(gpu, mem, row):
    kind, g, key = row.kind, row.g, R.family_key(row)
    check_iterations(gpu, row)
    lin = kind != 'wgrad'
    with tuning_env(**row.env):
        # ---- 1. integer pass ----
        di = cached(('int', g), lambda: R.int_inputs(g))
        iref, irb, _ = refs(kind, g, di, 'int')
        prev = di['prev'][R.base_kind(kind)]
        p = Product(gpu, kind, g, row.view, di)
        outs = [p.out()]
        exact(key, p.call(outs[-1]), iref, "integers, plain", at=(kind, g))
        if lin:
            for act in ('lrelu', 'relu'):
                outs.append(p.out())
                exact(key, p.call(outs[-1], act, bias=True), R.act64(irb, act), "integers, bias + %s" % act, at=(kind, g), zero_sign=act != 'relu')
        outs.append(p.out(prev))
        exact(key, p.call(outs[-1], accumulate=True), prev + iref, "integers, accumulate", at=(kind, g))
        p.settle((R.row_id(row), "integer pass"), outs)
        # ---- 2. real pass ----
        dr = cached(('real', g), lambda: R.real_inputs(g))
        r0, rb, M = refs(kind, g, dr, 'real')
        prev = dr['prev'][R.base_kind(kind)]
        p = Product(gpu, kind, g, row.view, dr)
        o1, o2, o3, o4 = p.out(), p.out(), p.out(), p.out(prev)
        got = p.call(o1, bias=lin)
        note(key, got, rb, M, "real", at=(kind, g))
        exact(key, p.call(o2, bias=lin), got, "real, repeated call", at=(kind, g))
        inc = p.call(o3) if lin else got
        exact(key, p.call(o4, accumulate=True), (prev + inc).astype(np.float32), "real, accumulate == fl32(previous + increment)", at=(kind, g))
        outs = [o1, o2, o3, o4]
        if row.kernel == 'fanin_s1' and kind == 'fwd' and g == (2, 64, 128, 128, 1, 5, 1, 2):      # g_out's own activation
            outs.append(p.out())
            th = p.call(outs[-1], 'tanh', bias=True)
            want = np.tanh(got.astype(np.float64))
            w = R.worst(th, want, np.maximum(np.abs(want), 2.0 ** -126))
            TANH[0] = max(TANH[0], w)
            print("tanh of the kernel's own linear output: worst %.3f units (bound %d)" % (w, K_LIBM['in_fwd_tanh']))
            assert np.isfinite(th).all() and w <= K_LIBM['in_fwd_tanh'], w
        p.settle((R.row_id(row), "real pass"), outs)


@pytest.mark.parametrize("row", [r for r in R.ROWS if r.kind != 'pool'], ids=R.row_id)
def test_row_agrees_with_the_general_kernel(gpu, mem, row):
    """every thin kernel against the general kernel it replaces (GHM_NO_THIN=1), inside twice the bound"""
    kind, g, key = row.kind, row.g, R.family_key(row)
    lin = kind != 'wgrad'
    dr = cached(('real', g), lambda: R.real_inputs(g))
    r0, rb, M = refs(kind, g, dr, 'real')
    p = Product(gpu, kind, g, row.view, dr)
    o1, o2 = p.out(), p.out()
    with tuning_env(**row.env):
        thin = p.call(o1, bias=lin)
    with tuning_env(**dict(row.env, GHM_NO_THIN='1')):
        general = p.call(o2, bias=lin)
    print("%s: the general kernel stands %.3f x 2^-24 M from the reference, the thin kernel %.3f" % (R.row_id(row), R.worst(general, rb, M), R.worst(thin, rb, M)))
    note(key, thin, general.astype(np.float64), M, "real, against GHM_NO_THIN=1", at=(kind, g), k=2 * R.K_BOUND[key], record=False)
    p.settle((R.row_id(row), "general kernel"), [o1, o2])


@pytest.mark.parametrize("row", [r for r in R.ROWS if r.kind == 'pool'], ids=R.row_id)
def test_pooled_row(gpu, mem, row):
    g, key = row.g, ('fanout', 'fwd')
    check_iterations(gpu, row)
    with tuning_env(**row.env):
        di = cached(('int', g), lambda: R.int_inputs(g))
        _, irb, _ = refs('fwd', g, di, 'int')
        p = Product(gpu, 'pool', g, row.view, di)
        outs = []
        for act in ('lrelu', 'relu'):
            want, wmask = R.pool_ref(R.act64(irb, act))
            tied = (np.unpackbits((wmask & 15)[..., None], axis=-1).sum(-1) > 1).mean()
            assert tied > 0.01, "the integer inputs must produce tied windows"
            o, m = p.out(), p.mask()
            pooled, mask = p.call_pool(o, m, act)
            exact(key, pooled, want, "integers, pooled bias + %s" % act, at=('pool', g), zero_sign=act != 'relu')
            assert np.array_equal(mask, wmask), ("integers, %s: %d mask bytes differ (%.0f %% of the windows are tied)"
                                                 % (act, (mask != wmask).sum(), 100 * tied))
            outs += [o, m]
        p.settle((R.row_id(row), "integer pass"), outs)
        dr = cached(('real', g), lambda: R.real_inputs(g))
        _, rb, M = refs('fwd', g, dr, 'real')
        p = Product(gpu, 'pool', g, row.view, dr)
        o1, m1, o2, m2 = p.out(), p.mask(), p.out(), p.mask()
        pooled, mask = p.call_pool(o1, m1, 'lrelu')
        note(key, pooled, R.pool_ref(R.act64(rb, 'lrelu'))[0], R.pool_ref(M)[0], "real, pooled", at=('pool', g))
        again, mask2 = p.call_pool(o2, m2, 'lrelu')
        exact(key, again, pooled, "real, repeated call", at=('pool', g))
        assert np.array_equal(mask, mask2)
        # the unpooled fan-out forward of the same inputs, pooled on the host: the same accumulators, so the same bits and mask
        full = V(gpu, R.shapes(g)[2], 'whole')
        gpu[1].conv2d_fwd(p.desc, p.x.t, p.w.t, p.bias.t, full.t, 'lrelu', R.SLOPE)
        want, wmask = R.pool_ref(full.numpy())
        exact(key, pooled, want, "real, pooled == max-pool of the unpooled forward", at=('pool', g))
        assert np.array_equal(mask, wmask)
        p.settle((R.row_id(row), "real pass"), [o1, m1, o2, m2, full])


@pytest.mark.parametrize("mode", R.Q_MODES)
@pytest.mark.parametrize("q", R.Q_ROWS, ids=lambda q: "%s-%s" % (q[0], "x".join(str(v) for v in q[1])))
def test_q_epilogue(gpu, mem, q, mode):
    """every plane of the q output == pieces(fp32 output of the same call); the q-only call gives the same planes; the fp32
    output is that of the plain entry point"""
    kind, g, ks = q
    dev, ops, D = gpu
    key = ('fanout', 'fwd')
    dr = cached(('real', g), lambda: R.real_inputs(g))
    with tuning_env(**R.Q_ENV):
        p = Product(gpu, kind, g, 'whole', dr)
        assert ops.thin_fwd_q_supported(p.desc, 'lrelu', kind == 'pool', mode)
        shape = R.out_shape(kind, g)
        plain, outs = p.out(), []
        if kind == 'fwd':
            y0 = p.call(plain, 'lrelu', bias=True)
        else:
            m0 = p.mask()
            y0, mask0 = p.call_pool(plain, m0, 'lrelu')
            outs.append(m0)
        for view in ('slice', 'offset'):
            o, outq, only = p.out(), QV(gpu, shape, mode, view), QV(gpu, shape, mode, view)
            if kind == 'fwd':
                ops.conv2d_fwd_thin_q(p.desc, p.x.t, p.w.t, p.bias.t, o.t, outq.q, 'lrelu', R.SLOPE)
                ops.conv2d_fwd_thin_q(p.desc, p.x.t, p.w.t, p.bias.t, None, only.q, 'lrelu', R.SLOPE)
            else:
                m1, m2 = p.mask(), p.mask()
                ops.conv2d_fwd_pool_thin_q(p.desc, p.x.t, p.w.t, p.bias.t, o.t, m1.ptr, outq.q, 'lrelu', R.SLOPE)
                ops.conv2d_fwd_pool_thin_q(p.desc, p.x.t, p.w.t, p.bias.t, None, m2.ptr, only.q, 'lrelu', R.SLOPE)
                assert np.array_equal(p.mask_bytes(m1), mask0) and np.array_equal(p.mask_bytes(m2), mask0)
                outs += [m1, m2]
            y = o.numpy()
            exact(key, y, y0, "%s %s: fp32 output of the q call == the plain call" % (mode, view), at=(kind, g))
            for i, (want, have, alone) in enumerate(zip(R.pieces(y, mode), outq.pieces(), only.pieces())):
                exact(key, have, want, "%s %s: q piece %d == pieces(fp32 output)" % (mode, view, i), at=(kind, g))
                exact(key, alone, want, "%s %s: q-only piece %d" % (mode, view, i), at=(kind, g))
            clean((q, mode, view, "q outputs"), outq, only)
            outs.append(o)
            for t in (outq, only):
                dev.free(t.ptr)
        p.settle((q, mode), outs + [plain])


@pytest.mark.parametrize("entry", R.MISALIGNED, ids=lambda e: "%s-%s" % (e[0], "x".join(str(v) for v in e[1])))
def test_output_four_bytes_in_is_not_given_to_the_vector_stores(gpu, mem, entry):
    """the alignment guard of thin_fanout_fwd_ok / thin_fanout_dgrad_ok / thin_fanout_fwd_pool_ok"""
    kind, g = entry
    key = ('fanout', R.base_kind(kind))
    if kind == 'pool':
        dr = cached(('real', g), lambda: R.real_inputs(g))
        p = Product(gpu, 'pool', g, 'whole', dr, out_view='off4')
        o, m = p.out(), p.mask()
        with pytest.raises(GhmError, match="aligned"):
            p.call_pool(o, m, 'lrelu')
        assert o.t.ptr % 8 == 4 and np.isnan(o.numpy()).all()                   # nothing was launched: all of it is still canary
        assert (np.ascontiguousarray(p.mask_bytes(m)).ravel().view(np.uint16) == Q.CANARY).all()
        p.settle((entry, "refused"), [o, m])
        return
    di, dr = cached(('int', g), lambda: R.int_inputs(g)), cached(('real', g), lambda: R.real_inputs(g))
    iref, irb, _ = refs(kind, g, di, 'int')
    p = Product(gpu, kind, g, 'whole', di, out_view='off4')
    outs = [p.out(), p.out(), p.out(di['prev'][R.base_kind(kind)])]
    assert outs[0].t.ptr % 16 == 4
    exact(key, p.call(outs[0]), iref, "4 bytes in: integers, plain", at=(kind, g))
    exact(key, p.call(outs[1], 'lrelu', bias=True), R.act64(irb, 'lrelu'), "4 bytes in: integers, bias + lrelu", at=(kind, g))
    exact(key, p.call(outs[2], accumulate=True), di['prev'][R.base_kind(kind)] + iref, "4 bytes in: integers, accumulate", at=(kind, g))
    p.settle((entry, "integer pass"), outs)
    r0, rb, M = refs(kind, g, dr, 'real')
    p = Product(gpu, kind, g, 'whole', dr, out_view='off4')
    o1, o2, o3 = p.out(), p.out(), V(gpu, R.out_shape(kind, g), 'whole')
    got = p.call(o1, bias=True)
    assert np.isfinite(got).all() and R.rel(got, rb) <= R.REL_L2
    thin = p.call(o3, bias=True)                        # the aligned view: the thin kernel
    with tuning_env(GHM_NO_THIN='1'):
        general = p.call(o2, bias=True)
    exact(key, got, general, "4 bytes in: the general kernel's bits", at=(kind, g))
    # (the bits cannot say WHICH kernel ran: igemm_kernel and the one-thread-per-pixel data gradient run the same fmaf steps in the
    # same order as fanout_kernel's MFMAs and add the bias last, as it does.  What this row holds is that the call is served, right
    # to the bit of the general kernel, with nothing written outside the view 4 bytes in)
    print("%s: the thin kernel's bits %s the general kernel's" % (kind, "equal" if Q.bits_equal(thin, general) else "differ from"))
    p.settle((entry, "real pass"), [o1, o2, o3])
