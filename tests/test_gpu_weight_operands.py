"""The nine kernels that derive the convolutions' weight operands from the fp32 master weights, and the tables that drive their
per-net forms, bit for bit: the fp32 transposed copy, the bf16 / fp16 packs, the split packs of two and three planes, the collapsed
up-sample weights with their tiled bias (mode 0: nearest -> 5x5, mode 1: bilinear -> 3x3) and the expansion of their gradient,
each in its single-layer form and in its batched (table) form -- the one every training step runs.  The definitions, the row
tables (each row says which branch or edge it reaches) and the input sets are tests/weight_operand_ref.py;
tests/test_weight_operand_ref.py holds them to account on the CPU, the real table builders of device.Ops included.

Per call:
  1. value: transposes and every halfword of every plane of a pack, padding included, bit for bit against the definition; collapse
     and expand bit for bit against the float32 restatement of the kernel's sums, per element |got - ref| <= k 2^-24 M against the
     float64 definition (k = the additions of that element, M = the sum of |term|), rel-L2 <= 1e-5; the accumulating expand equals
     fl32(previous + increment), the increment being what the plain call wrote; bias4 bit for bit;
  2. the batched form, all rows of a kind in one table (the packs in an order whose neighbours differ in T, rpad and transposed),
     the table reversed, and n = 1 tables of the first and the last row: every item bit-identical to the single-layer form's;
  3. nothing else is written: every destination is a region of a NaN-canary-filled allocation (batched: all of them carved from
     ONE allocation, 16 canary bytes apart), no canary changes, with bias = None bias4 is all canary, sources (views 1 or 3 floats
     into their allocation, as parameters in the flat ParamStore buffer are) and tables are bit-unchanged;
  4. the engine's order in one stream: every buffer and table made first, then the collapse launch and the pack launches on the
     collapsed buffers issued back to back -- no allocation, copy or sync between them -- and one sync behind the last;
  5. the tables the engine really builds (test_the_operands_the_engine_derives): after two train steps and a forward-only call of
     the LP_STEP model, every forward operand -- wpc, bias4, every pack of plan._lp_wq, plain and transposed -- is the transform of
     the CURRENT master weights in bits.  The fp32 transposed copies (store.transposed(W), wpcT) are refreshed in the middle of a
     train step, behind the forward pass and in front of the backward pass and the update, and by nothing else: after the second
     step they are the transform of the weights BEFORE that step's update (= after the first step's), never of the initial ones,
     and the forward-only call leaves them alone.

Measured on the MI355X, max over all rows of |got - ref| / (2^-24 M) against the k asserted per element (the additions of that
element), the rel-L2 where it is asserted, and the number of comparisons (the module prints the three when it finishes):
  transpose / batched            bit for bit                                               0         12 / 14
  lp_pack bf16, f16 / batched    every halfword bit for bit                                0         21 each / 22 each
  split_pack x3, x2 / batched    every halfword of every plane bit for bit                 0         20 each / 22 each
  q_pack bf16, f16               the conversion classes: the halfwords of lp_pack_weights  0         1 each
  collapse                       1.95 of 0 .. 3 (mode 0: 1, 2 or 4 terms); == restate32    3.6e-08   12
  collapse batched               mode 0 the same; mode 1 2.68 of 0 .. 8 (0 .. 9 terms)     4.4e-08   44
  bias4 / batched                bit for bit                                               0         4 / 9
  expand / accumulate            2.20 of 3 / 2.20 of 4; == restate32, == fl32(prev + inc)  4.0e-08   8 / 12
  expand batched / accumulate    mode 0 the same; mode 1 2.23 of 8 / 2.04 of 9             5.5e-08   24 / 36
  packs of wpc, engine order     bit for bit in the four dtypes                            0         10 each
  engine wpc, bias4              bit for bit, the current weights                          0         15 / 15
  engine packs bf16 / bf16x3     bit for bit, the current weights: 20 + 19 / 14 + 11 (plain + transposed)      39 / 25
  engine transposed copies       the weights before the second update, bit for bit: f32 11 + 5 (of wpc), bf16 0 + 1, bf16x3 3 + 2
No conversion class disagrees with the definition: denormals are not flushed, by ghm_q_pack or by the weight packs
(0x00018000 -> 0x0002, 0x007fffff -> 0x0080), ties go to even, FLT_MAX and 65520 go to inf.
No kernel needed a fix.  Changed with this module, all on the host: the five batched entry points refuse a null ctx or table
(ghm_split_pack_batched did already); ghm_lp_pack_weights / ghm_split_pack_weights refuse a pack that is not 16-byte aligned, and
device.Ops.lp_pack_table does the same for the batched forms, whose entry points cannot read the device table; include/ghm.h called
the collapse record "40-byte" -- it is 48 bytes in the kernel and in device.Ops.collapse_table, the header says so now and the entry
points of the collapse and expand tables assert their record sizes at compile time, as the other two did.
Wall time on the MI355X: this module 1.6 s, 0.9 s of it in its tests (the three engine cases 0.5 s).
"""
import numpy as np
import pytest

from gan_heightmaps_amd._lib import GhmError, call
from tests import canary
from tests import weight_operand_ref as R

pytestmark = pytest.mark.gpu

_REF = {}
LEDGER = canary.Ledger(lambda op, w, r, n: "measured %-22s worst k %7.3f  rel-L2 %.2e  (%d comparisons)" % (op, w, r, n))
gpu, mem = canary.fixtures(LEDGER, _REF, loss_scale=True)
V, unchanged, fl32_sum, exact = canary.View.free, canary.unchanged, canary.fl32_sum, LEDGER.exact
DTYPES = R.LP_DTYPES + R.SPLIT_DTYPES
GAP = 16            # canary bytes between neighbouring destinations of a table


def ids(rows):
    return [str(r) for r, _ in rows]


class Arena:
    """regions of the given byte sizes carved from ONE canary-filled allocation, GAP canary bytes in front of each and a tail
    behind the last; with 16-byte multiples as sizes every region is 16-byte aligned"""

    def __init__(self, gpu, sizes, tail=64):
        self.dev, _, self.D = gpu
        self.sizes = [int(s) for s in sizes]
        self.offs, o = [], 0
        for s in self.sizes:
            o += GAP
            self.offs.append(o)
            o += s
        self.total = (o + tail + 1) // 2 * 2
        self.base = self.dev.alloc(self.total)
        assert self.base % 16 == 0
        self.inside = np.zeros(self.total // 2, bool)
        for o, s in zip(self.offs, self.sizes):
            assert o % 4 == 0 and s % 2 == 0
            self.inside[o // 2:(o + s) // 2] = True
        self.fill()

    def fill(self):
        R.canary_fill(self.dev, self.base, self.total)

    def ptr(self, i):
        return self.base + self.offs[i]

    def f32(self, i):
        return self.D.DevTensor(self.dev, self.ptr(i), (1, self.sizes[i] // 4, 1, 1))

    def read(self, i, dtype=np.uint16):
        out = np.empty(self.sizes[i] // np.dtype(dtype).itemsize, dtype)
        self.dev.d2h(out, self.ptr(i), self.sizes[i])
        return out

    def stray(self):
        return R.canary_changed(self.dev, self.base, self.total, self.inside)

    def all_canary(self, i):
        return bool((self.read(i) == R.CANARY).all())


def src(gpu, data, i=0):
    """an fp32 source 1 or 3 floats into its allocation"""
    data = np.ascontiguousarray(data, np.float32)
    return V(gpu, (data.size,), (1 if i % 2 == 0 else 3, 0), data.reshape(-1))


def table_bytes(dev, table, size):
    raw = np.empty(table[1] * size, np.uint8)
    dev.d2h(raw, table[0], raw.nbytes)
    return raw


def same_halfwords(op, got, want, what):
    LEDGER.record(op)
    assert got.shape == want.shape, (op, what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        pytest.fail("%s %s: %d of %d halfwords differ, first at %d (unit %d, lane %d): got %#06x, expected %#06x"
                    % (op, what, bad.size, got.size, i, i // 8, i % 8, got[i], want[i]))


def hold_k(op, got, ref, M, k, what):
    """per element |got - ref| <= k 2^-24 M with k the element's own count, and the rel-L2; the figures printed first"""
    got, ref, M = np.asarray(got), np.asarray(ref, np.float64), np.asarray(M, np.float64)
    w, r = R.worst(got, ref, M), R.rel(got, ref)
    print("%s %s: worst k %.3f (bound %d .. %d per element)  rel-L2 %.2e" % (op, what, w, k.min(), k.max(), r))
    LEDGER.record(op, w, r)
    assert np.isfinite(got).all(), (op, what)
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > k * R.U * M
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        pytest.fail("%s %s: %d elements over their bound, first %s: got %r ref %r, k = %d" % (op, what, bad.sum(), i, got[i], ref[i], k[i]))
    assert r <= R.REL_L2, (op, what, r)


def pack_op(dtype):
    return 'split_pack/' + dtype if dtype in R.SPLIT_DTYPES else 'lp_pack/' + dtype


def pack_ref(row, dtype):
    key = ('pack', row, dtype)
    if key not in _REF:
        wp = R.pack_inputs(row, dtype)
        _REF[key] = (wp, R.lp_pack(wp, *row, dtype))
    return _REF[key]


def desc_of(D, row):
    C, K, kh, kw = R.pack_desc_args(row)
    return D.conv_desc(1, C, 8, 8, K, kh, kw, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# packs
def single_pack(gpu, row, dtype, i=0):
    """ghm_lp_pack_weights / ghm_split_pack_weights on one row -> the halfwords, every check of a single call made"""
    dev, ops, D = gpu
    red, T, rows, tr = row
    wp, want = pack_ref(row, dtype)
    what = "%s %s" % (row, dtype)
    d = desc_of(D, row)
    nbytes = ops.lp_weight_bytes(d, bool(tr), dtype)
    assert nbytes == R.weight_bytes(red, T, rows, dtype) == 2 * want.size, what
    s, dst = src(gpu, wp, i), Arena(gpu, [nbytes])
    assert dst.ptr(0) % 16 == 0
    ops.lp_pack_weights(d, s.t, dst.ptr(0), dtype, bool(tr))
    got = dst.read(0)
    same_halfwords(pack_op(dtype), got, want, what + " single layer")
    assert dst.stray().size == 0, (what, "written outside the pack")
    unchanged(what, s)
    dev.free(s.ptr)
    dev.free(dst.base)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row,why", R.PACK_ROWS, ids=ids(R.PACK_ROWS))
def test_pack_single_layer(gpu, mem, row, why, dtype):
    """ghm_lp_pack_weights (bf16, f16) / ghm_split_pack_weights (3 and 2 planes): every halfword of every plane, the zero rows and
    the zero channel blocks included, inside a destination exactly ghm_lp_weight_bytes / ghm_split_weight_bytes long"""
    single_pack(gpu, row, dtype)


def pack_table(gpu, rows, dtype, what):
    """ghm_lp_pack_batched / ghm_split_pack_batched on a table of ``rows`` in this order -> the halfwords per item"""
    dev, ops, D = gpu
    srcs = [src(gpu, pack_ref(r, dtype)[0], i) for i, r in enumerate(rows)]
    dst = Arena(gpu, [R.weight_bytes(*r[:3], dtype) for r in rows])
    items = [(s.t if i % 2 else s.t.ptr, dst.ptr(i), r[0], r[1], r[2], r[3]) for i, (s, r) in enumerate(zip(srcs, rows))]
    table = ops.lp_pack_table(items)
    assert table[2] == sum(R.pack_blocks(*r[:3]) for r in rows) <= 290
    before = table_bytes(dev, table, R.LP_RECORD[1])
    ops.lp_pack_batched(table, dtype)
    got = [dst.read(i) for i in range(len(rows))]
    assert dst.stray().size == 0, (what, dtype, "written outside the packs of the table")
    assert np.array_equal(table_bytes(dev, table, R.LP_RECORD[1]), before), (what, "the table was modified")
    unchanged(what, *srcs)
    for s in srcs:
        dev.free(s.ptr)
    dev.free(dst.base)
    dev.free(table[0])
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_batched(gpu, mem, dtype):
    """every row of the pack table in ONE launch, neighbours differing in T, rpad and transposed; the table reversed; n = 1 tables
    of the first and the last row: each item is the reference's and the single-layer form's halfwords"""
    rows = [R.PACK_ROWS[i][0] for i in R.PACK_TABLE_ORDER]
    single = {r: single_pack(gpu, r, dtype, i) for i, r in enumerate(rows)}
    for order, name in ((rows, "table"), (rows[::-1], "reversed table"), (rows[:1], "n = 1, first row"), (rows[-1:], "n = 1, last row")):
        got = pack_table(gpu, order, dtype, name)
        for r, g in zip(order, got):
            same_halfwords(pack_op(dtype) + ' batched', g, pack_ref(r, dtype)[1], "%s %s in the %s" % (r, dtype, name))
            assert np.array_equal(g, single[r]), (r, dtype, name, "differs from the single-layer form")


def test_weight_and_activation_operands_round_alike(gpu, mem):
    """the conversion classes through ghm_q_pack (the activation operand's producer) and through ghm_lp_pack_weights: the same
    halfwords, and those of the definition -- the two operands of one product round alike"""
    dev, ops, D = gpu
    for dtype, bits in (('bf16', R.bf16_special_bits()), ('f16', R.f16_special_bits())):
        m = -(-bits.size // 8)
        s = R.f32_source((8, 1, m), 7).reshape(-1)
        s[:bits.size] = bits.view(np.float32)
        with np.errstate(over='ignore'):
            want = R.halfwords(R.pieces(s, dtype)[0], dtype)
        x = V(gpu, (1, 8, 1, m), data=s.reshape(m, 8).T)            # channel j of pixel p = value 8 p + j
        q = Arena(gpu, [16 * m])
        ops.q_pack(x.t, D.QTensor(dev, q.ptr(0), (1, 8, 1, m), dtype))
        act = q.read(0)
        wsrc = src(gpu, s.reshape(m, 8).T.reshape(8, 1, m))         # wp[c][0][r] = value 8 r + c
        wq = Arena(gpu, [R.weight_bytes(8, 1, m, dtype)])
        ops.lp_pack_weights(D.conv_desc(1, 8, 8, 8, m, 1, 1, 1, 0), wsrc.t, wq.ptr(0), dtype, False)
        wgt = wq.read(0)[:8 * m]
        for i in np.flatnonzero((act != want) | (wgt != want))[:16]:
            print("%s value %#010x: q_pack %#06x, lp_pack_weights %#06x, definition %#06x" % (dtype, s.view(np.uint32)[i], act[i], wgt[i], want[i]))
        assert np.array_equal(act, wgt), (dtype, "the two producers round differently")
        same_halfwords('q_pack/' + dtype, act, want, "conversion classes")
        same_halfwords('lp_pack/' + dtype, wgt, want, "conversion classes")
        assert q.stray().size == 0 and wq.stray().size == 0
        unchanged(dtype, x, wsrc)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 transposes
def transpose_ref(row):
    key = ('transpose', row)
    if key not in _REF:
        wp = R.f32_source(row, 6)
        _REF[key] = (wp, R.transpose(wp).reshape(-1))
    return _REF[key]


def single_transpose(gpu, row, i=0):
    dev, ops, D = gpu
    C, T, K = row
    wp, want = transpose_ref(row)
    k = {1: 1, 4: 2, 9: 3, 25: 5}[T]
    s, dst = src(gpu, wp, i), Arena(gpu, [4 * wp.size])
    ops.transpose_weights(D.conv_desc(1, C, 8, 8, K, k, k, 1, 0), s.t, dst.f32(0))
    got = dst.read(0, np.float32)
    exact('transpose', got, want, "%s single layer" % (row,))
    assert dst.stray().size == 0, (row, "written outside wpT")
    unchanged(row, s)
    return got


@pytest.mark.parametrize("row,why", R.TRANSPOSE_ROWS, ids=ids(R.TRANSPOSE_ROWS))
def test_transpose_single_layer(gpu, mem, row, why):
    """ghm_conv2d_transpose_weights: wpT[k][T - 1 - tap][c] = wp[c][tap][k] bit for bit, ragged tiles on either side"""
    single_transpose(gpu, row)


def test_transpose_batched(gpu, mem):
    """ghm_transpose_weights_batched: all rows in one table, reversed, and n = 1 tables of the first and the last row"""
    dev, ops, D = gpu
    rows = [r for r, _ in R.TRANSPOSE_ROWS]
    single = {r: single_transpose(gpu, r, i) for i, r in enumerate(rows)}
    for order, name in ((rows, "table"), (rows[::-1], "reversed table"), (rows[:1], "n = 1, first row"), (rows[-1:], "n = 1, last row")):
        srcs = [src(gpu, transpose_ref(r)[0], i) for i, r in enumerate(order)]
        dst = Arena(gpu, [4 * r[0] * r[1] * r[2] for r in order])
        table = ops.transpose_table([(s.t, dst.f32(i)) + r for i, (s, r) in enumerate(zip(srcs, order))])
        assert table[2] == sum(R.transpose_blocks(*r) for r in order) <= 290
        before = table_bytes(dev, table, R.TRANSPOSE_RECORD[1])
        ops.transpose_weights_batched(table)
        for i, r in enumerate(order):
            got = dst.read(i, np.float32)
            exact('transpose batched', got, transpose_ref(r)[1], "%s in the %s" % (r, name))
            assert R.bits_equal(got, single[r]), (r, name, "differs from the single-layer form")
        assert dst.stray().size == 0, (name, "written outside the transposed copies of the table")
        assert np.array_equal(table_bytes(dev, table, R.TRANSPOSE_RECORD[1]), before), (name, "the table was modified")
        unchanged(name, *srcs)


# ---------------------------------------------------------------------------------------------------------------------
# collapse
def collapse_ref(row):
    key = ('collapse', row)
    if key not in _REF:
        C, K, mode, _ = row
        d = R.collapse_inputs(row)
        _REF[key] = dict(d, r32=R.restate32_collapse(d['wp'], mode), ref=R.collapse(d['wp'], mode), M=R.collapse_M(d['wp'], mode),
                         k=R.collapse_k(mode, C, K), b4=R.bias4(d['bias']) if d['bias'] is not None else None)
    return _REF[key]


def check_collapse(op, row, wpc, b4_region, what):
    """wpc: the float32 elements read back; b4_region: (arena, index) of bias4"""
    C, K, mode, has_bias = row
    d = collapse_ref(row)
    got = wpc.reshape(C, 9, 4, K)
    exact(op, got, d['r32'], what + " against the float32 restatement")
    hold_k(op, got, d['ref'], d['M'], d['k'], what)
    none = np.broadcast_to((R.collapse_terms(mode) == 0)[None, :, :, None], got.shape)
    assert not got[none].view(np.uint32).any(), (what, "an output without a term must be +0.0 in bits")
    arena, i = b4_region
    if has_bias:
        exact(op + ' bias4', arena.read(i, np.float32), d['b4'], what)
    else:
        assert arena.all_canary(i), (what, "bias = None: bias4 must keep its canary")
    return got


def collapse_srcs(gpu, row, i):
    d = collapse_ref(row)
    return src(gpu, d['wp'], i), (src(gpu, d['bias'], i + 1) if d['bias'] is not None else None)


def single_collapse(gpu, row, i=0):
    dev, ops, D = gpu
    C, K, mode, has_bias = row
    assert mode == 0
    w, b = collapse_srcs(gpu, row, i)
    dst = Arena(gpu, [4 * 36 * C * K, 4 * 4 * K])
    ops.upconv_collapse_weights(w.t, b.t if b is not None else None, dst.f32(0), dst.f32(1), C, K)
    got = check_collapse('collapse', row, dst.read(0, np.float32), (dst, 1), "%s single layer" % (row,))
    assert dst.stray().size == 0, (row, "written outside wpc / bias4")
    unchanged(row, *[v for v in (w, b) if v is not None])
    return got


@pytest.mark.parametrize("row,why", [r for r in R.COLLAPSE_ROWS if r[0][2] == 0], ids=ids([r for r in R.COLLAPSE_ROWS if r[0][2] == 0]))
def test_collapse_single_layer(gpu, mem, row, why):
    """ghm_upconv_collapse_weights (mode 0 only): wpc and bias4"""
    single_collapse(gpu, row)


def collapse_table_build(gpu, order):
    """sources, destinations and the device table of one ghm_upconv_collapse_batched launch over ``order``, nothing launched
    -> (arena of [wpc, bias4] per item, sources, table, the table's bytes)"""
    dev, ops, D = gpu
    srcs = [collapse_srcs(gpu, r, 2 * i) for i, r in enumerate(order)]
    dst = Arena(gpu, sum(([4 * 36 * r[0] * r[1], 16 * r[1]] for r in order), []))
    table = ops.collapse_table([(w.t, b.t if b is not None else None, dst.f32(2 * i), dst.f32(2 * i + 1), r[0], r[1], r[2])
                                for i, ((w, b), r) in enumerate(zip(srcs, order))])
    assert table[2] == sum(R.collapse_blocks(r[0], r[1]) for r in order)
    return dst, srcs, table, table_bytes(dev, table, R.COLLAPSE_RECORD[1])


def test_collapse_batched(gpu, mem):
    """ghm_upconv_collapse_batched, both modes: all rows in one table, reversed, n = 1 tables of the first and the last row"""
    dev, ops, D = gpu
    rows = [r for r, _ in R.COLLAPSE_ROWS]
    single = {r: single_collapse(gpu, r, i) for i, r in enumerate(rows) if r[2] == 0}
    for order, name in ((rows, "table"), (rows[::-1], "reversed table"), (rows[:1], "n = 1, first row"), (rows[-1:], "n = 1, last row")):
        assert max(R.collapse_blocks(r[0], r[1]) for r in order) <= 290
        dst, srcs, table, before = collapse_table_build(gpu, order)
        ops.upconv_collapse_batched(table)
        for i, r in enumerate(order):
            got = check_collapse('collapse batched', r, dst.read(2 * i, np.float32), (dst, 2 * i + 1), "%s in the %s" % (r, name))
            if r in single:
                assert R.bits_equal(got, single[r]), (r, name, "differs from the single-layer form")
        assert dst.stray().size == 0, (name, "written outside the collapsed weights of the table")
        assert np.array_equal(table_bytes(dev, table, R.COLLAPSE_RECORD[1]), before), (name, "the table was modified")
        unchanged(name, *[v for pair in srcs for v in pair if v is not None])


# ---------------------------------------------------------------------------------------------------------------------
# expand
def expand_ref(row):
    key = ('expand', row)
    if key not in _REF:
        C, K, mode = row
        d = R.expand_inputs(row)
        _REF[key] = dict(d, r32=R.restate32_expand(d['dwpc'], mode), ref=R.expand(d['dwpc'], mode), M=R.expand_M(d['dwpc'], mode),
                         Macc=R.expand_M(d['dwpc'], mode, d['prev']))
    return _REF[key]


def check_expand(op, row, plain, acc, what):
    C, K, mode = row
    d = expand_ref(row)
    shape = d['prev'].shape
    plain, acc = plain.reshape(shape), acc.reshape(shape)
    exact(op, plain, d['r32'], what + " against the float32 restatement")
    hold_k(op, plain, d['ref'], d['M'], R.expand_k(mode, C, K, False), what)
    exact(op + ' accumulate', acc, fl32_sum(d['prev'], plain), what + ": fl32(previous + increment)")
    exact(op + ' accumulate', acc, R.restate32_expand(d['dwpc'], mode, d['prev']), what + " accumulating, against the restatement")
    hold_k(op + ' accumulate', acc, d['ref'] + d['prev'], d['Macc'], R.expand_k(mode, C, K, True), what + " accumulating")
    return plain


def single_expand(gpu, row, i=0):
    dev, ops, D = gpu
    C, K, mode = row
    assert mode == 0
    d = expand_ref(row)
    g = src(gpu, d['dwpc'], i)
    dst = Arena(gpu, [4 * 25 * C * K, 4 * 25 * C * K])
    dst.f32(1).set(d['prev'].reshape(-1))
    ops.upconv_expand_wgrad(g.t, dst.f32(0), C, K, False)
    ops.upconv_expand_wgrad(g.t, dst.f32(1), C, K, True)
    got = check_expand('expand', row, dst.read(0, np.float32), dst.read(1, np.float32), "%s single layer" % (row,))
    assert dst.stray().size == 0, (row, "written outside dwp5")
    unchanged(row, g)
    return got


@pytest.mark.parametrize("row,why", [r for r in R.EXPAND_ROWS if r[0][2] == 0], ids=ids([r for r in R.EXPAND_ROWS if r[0][2] == 0]))
def test_expand_single_layer(gpu, mem, row, why):
    """ghm_upconv_expand_wgrad (mode 0 only), plain and accumulating"""
    single_expand(gpu, row)


def test_expand_batched(gpu, mem):
    """ghm_upconv_expand_batched, both modes, plain and accumulating: all rows in one table, reversed, n = 1 tables of the first
    and the last row; a mode-1 item's trailing blocks write nothing"""
    dev, ops, D = gpu
    rows = [r for r, _ in R.EXPAND_ROWS]
    single = {r: single_expand(gpu, r, i) for i, r in enumerate(rows) if r[2] == 0}
    for order, name in ((rows, "table"), (rows[::-1], "reversed table"), (rows[:1], "n = 1, first row"), (rows[-1:], "n = 1, last row")):
        srcs = [src(gpu, expand_ref(r)['dwpc'], i) for i, r in enumerate(order)]
        sizes = [4 * R.TAPS[r[2]] ** 2 * r[0] * r[1] for r in order]
        res = []
        for accumulate in (False, True):
            dst = Arena(gpu, sizes)
            if accumulate:
                for i, r in enumerate(order):
                    dst.f32(i).set(expand_ref(r)['prev'].reshape(-1))
            table = ops.expand_table([(s.t, dst.f32(i)) + r for i, (s, r) in enumerate(zip(srcs, order))])
            assert table[2] == sum(R.expand_blocks(*r) for r in order) <= 290
            before = table_bytes(dev, table, R.EXPAND_RECORD[1])
            ops.upconv_expand_batched(table, accumulate)
            res.append([dst.read(i, np.float32) for i in range(len(order))])
            assert dst.stray().size == 0, (name, accumulate, "written outside the gradients of the table")
            assert np.array_equal(table_bytes(dev, table, R.EXPAND_RECORD[1]), before), (name, "the table was modified")
        for i, r in enumerate(order):
            got = check_expand('expand batched', r, res[0][i], res[1][i], "%s in the %s" % (r, name))
            if r in single:
                assert R.bits_equal(got, single[r]), (r, name, "differs from the single-layer form")
        unchanged(name, *srcs)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_collapse_then_pack_in_one_stream(gpu, mem, dtype):
    """the head of the engine's forward program: ghm_upconv_collapse_batched, then the pack launches that read the collapsed
    buffers.  Sources, destinations and the three device tables exist before the first launch (building a table allocates and
    uploads, and an upload drains the stream); then the three launches are issued back to back with no allocation, copy or sync
    between them, and the stream is synced once behind the last.  Every pack -- plain (red = C, rows = 4 K) and transposed
    (red = 4 K, rows = C) -- is lp_pack(restate32_collapse(wp)) in bits.  Two pack tables, so that no launch is larger than 290
    blocks."""
    dev, ops, D = gpu
    rows = [r for r, _ in R.COLLAPSE_ROWS]
    geo = [(r, tr, (4 * r[1], 9, r[0], 1) if tr else (r[0], 9, 4 * r[1], 0)) for r in rows for tr in (0, 1)]
    big = max(geo, key=lambda g: R.pack_blocks(*g[2][:3]))
    groups = [[g for g in geo if g is not big], [big]]
    arenas = [Arena(gpu, [R.weight_bytes(*g[2][:3], dtype) for g in grp]) for grp in groups]
    dst, srcs, ctable, cbefore = collapse_table_build(gpu, rows)
    tables = []
    for grp, ar in zip(groups, arenas):
        items = [(dst.f32(2 * rows.index(r)), ar.ptr(i)) + p for i, (r, tr, p) in enumerate(grp)]
        tables.append(ops.lp_pack_table(items))
        assert tables[-1][2] <= 290
    before = [table_bytes(dev, t, R.LP_RECORD[1]) for t in tables]
    dev.sync()
    # ---- the three launches, and nothing else, between these two syncs ----
    ops.upconv_collapse_batched(ctable)
    ops.lp_pack_batched(tables[0], dtype)
    ops.lp_pack_batched(tables[1], dtype)
    dev.sync()
    assert np.array_equal(table_bytes(dev, ctable, R.COLLAPSE_RECORD[1]), cbefore), "the collapse table was modified"
    for t, b in zip(tables, before):
        assert np.array_equal(table_bytes(dev, t, R.LP_RECORD[1]), b), "a pack table was modified"
    for grp, ar in zip(groups, arenas):
        for i, (r, tr, p) in enumerate(grp):
            wpc = collapse_ref(r)['r32'].reshape(r[0], 9, 4 * r[1])
            same_halfwords(pack_op(dtype) + ' of wpc', ar.read(i), R.lp_pack(wpc, *p, dtype), "%s %s %s" % (r, "transposed" if tr else "plain", dtype))
        assert ar.stray().size == 0
    for i, r in enumerate(rows):
        exact('collapse batched', dst.read(2 * i, np.float32).reshape(r[0], 9, 4, r[1]), collapse_ref(r)['r32'], "%s in front of the packs" % (r,))
    assert dst.stray().size == 0
    unchanged("engine order", *[v for pair in srcs for v in pair if v is not None])


# ---------------------------------------------------------------------------------------------------------------------
def test_table_entry_points_refuse_null_and_misaligned_arguments(gpu, mem):
    """the five batched entry points check ctx and table on the host; ghm_lp_pack_weights / ghm_split_pack_weights and the table
    builder refuse a pack that is not 16-byte aligned.  An error, and nothing launched"""
    dev, ops, D = gpu
    some = dev.alloc(256)
    for name, extra in (("ghm_lp_pack_batched", (1,)), ("ghm_split_pack_batched", (3,)), ("ghm_transpose_weights_batched", ()),
                        ("ghm_upconv_collapse_batched", ()), ("ghm_upconv_expand_batched", (0,))):
        with pytest.raises(GhmError, match="null argument"):
            call(name, None, some, 1, 1, *extra)
        with pytest.raises(GhmError, match="null argument"):
            call(name, dev.h, None, 1, 1, *extra)
    row = (16, 9, 128, 0)
    d = desc_of(D, row)
    s, dst = src(gpu, pack_ref(row, 'bf16')[0]), Arena(gpu, [R.weight_bytes(16, 9, 128, 'bf16x3') + 16])
    for dtype in DTYPES:
        for off in (2, 4, 8):
            with pytest.raises(GhmError, match="16-byte aligned"):
                ops.lp_pack_weights(d, s.t, dst.ptr(0) + off, dtype, False)
    with pytest.raises(GhmError, match="null argument"):
        ops.lp_pack_weights(d, s.t, None, 'bf16', False)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.lp_pack_table([(s.t, dst.ptr(0) + 8, 16, 9, 128, 0)])
    dev.sync()
    assert dst.all_canary(0) and dst.stray().size == 0, "a refused call wrote"
    unchanged("refused", s)


# ---------------------------------------------------------------------------------------------------------------------
# the tables the engine really builds
def listed_transposes(plan):
    """the items NetPlan.emit_transposes puts into its table: [(source, transposed copy, C, T, K)]"""
    got = []
    plan.ops.transpose_table = lambda items: got.extend(items) or (0, 0, 0)         # shadows the method for one call
    try:
        plan.emit_transposes([], set())
    finally:
        del plan.ops.transpose_table
    return got


@pytest.mark.parametrize("dtype", ["f32", "bf16", "bf16x3"])
def test_the_operands_the_engine_derives(gpu, mem, dtype):
    """two train steps of the LP_STEP model (collapsed, stride-1 and stride-2 layers on the low-precision kernels), then a
    forward-only call; then every item of the plans' own structures against the transform of the downloaded master weights.
    Forward operands: the CURRENT weights, in bits.  The fp32 transposed copies: the weights the second step's backward pass saw
    -- those BEFORE its update -- because emit_transposes sits between the step's forward and backward passes and the update comes
    last; a forward-only program has no such launch"""
    from oracle import step as ostep
    from tests.gpu_common import LP_STEP
    from tests.gpu_common import build_model
    dev, ops, D = gpu
    cfg = ostep.default_cfg(**LP_STEP)
    model = build_model(cfg, 7, dev, dtype=dtype)
    eng = model.engine

    def weights():
        eng.sync()
        return {k: st.w.numpy().reshape(-1).copy() for k, st in eng.stores.items()}
    w0 = weights()
    losses = []
    snaps = [w0]
    for it in range(2):
        Z, X, Y = ostep.synthetic_batch(4, cfg, seed=300 + it)
        losses.append(model.train_fn(Z, X, Y))
        snaps.append(weights())
    w1, w2 = snaps[1], snaps[2]
    Z, X, Y = ostep.synthetic_batch(4, cfg, seed=302)
    losses.append(model.loss_fn(Z, X, Y))
    assert np.isfinite(np.asarray(losses, np.float64)).all()
    now = weights()
    assert all(np.array_equal(now[k].view(np.uint32), w2[k].view(np.uint32)) for k in w2), "a forward-only call moved the weights"
    b = eng.built(4)
    n_items = dict(wpc=0, bias4=0, pack=0, pack_transposed=0, transpose=0, transpose_of_wpc=0)
    when = set()
    for plan, key in ((b.G, 'dcgan_gen'), (b.D, 'dcgan_disc'), (b.U, 'p2p_gen'), (b.P, 'p2p_disc')):
        st = eng.stores[key]
        assert plan.store is st

        def master(w, p):
            assert p.index[0] == 'w'
            return w[key][p.index[1]:p.index[1] + int(np.prod(p.shape))]

        def packed(w, W):
            K, C, kh, kw = W.shape
            return master(w, W).reshape(C, kh * kw, K)
        ups = {}
        for n in plan.order:
            if n.op != 'upconv':
                continue
            what = "%s %s %r" % (dtype, key, n)
            C, K, mode = n.inputs[0].shape[1], n.shape[1], n.attrs.get('mode', 0)
            assert n.layer.W.shape == (K, C, R.TAPS[mode], R.TAPS[mode])
            ups[n.aux['wpc'].ptr] = (n, C, K, mode)
            exact('engine wpc', n.aux['wpc'].numpy().reshape(C, 9, 4, K), R.restate32_collapse(packed(w2, n.layer.W), mode), what)
            exact('engine bias4', n.aux['b4'].numpy().reshape(-1), R.bias4(master(w2, n.layer.b)), what)
            n_items['wpc'] += 1
            n_items['bias4'] += 1
        # the packs of plan._lp_wq, found as NetPlan._plan_lp_packs lays them out
        seen = set()
        for n in plan.order:
            if n.op in ('conv', 'convpool'):
                d, pk = plan._desc(n, n.inputs[0].out, plan._full(n)), ('w', id(n.layer.W))
                wp = packed(w2, n.layer.W)
            elif n.op == 'upconv':
                d, pk = plan._upconv_desc(n, n.inputs[0].out), ('c', id(n.layer.W))
                _, C, K, mode = ups[n.aux['wpc'].ptr]
                wp = R.restate32_collapse(packed(w2, n.layer.W), mode).reshape(C, 9, 4 * K)
            else:
                continue
            T = d.kh * d.kw
            assert wp.shape == (d.C, T, d.K), (n, wp.shape, (d.C, T, d.K))
            for tr in (0, 1):
                if (pk, bool(tr)) not in plan._lp_wq or (pk, tr) in seen:
                    continue
                seen.add((pk, tr))
                red, rows = (d.K, d.C) if tr else (d.C, d.K)
                raw = np.empty(R.weight_bytes(red, T, rows, dtype) // 2, np.uint16)
                plan.dev.d2h(raw, plan._lp_wq[(pk, bool(tr))], raw.nbytes)
                same_halfwords('engine ' + pack_op(dtype), raw, R.lp_pack(wp, red, T, rows, tr, dtype), "%s %r %s" % (key, n, "transposed" if tr else "plain"))
                n_items['pack_transposed' if tr else 'pack'] += 1
        assert len(seen) == len(plan._lp_wq), (key, "a pack of plan._lp_wq was not visited")
        # the fp32 transposed copies refreshed in the middle of a train step
        for s, t, C, T, K in listed_transposes(plan):
            if s.ptr in ups:
                n, c_, k_, mode = ups[s.ptr]
                assert t.ptr == n.aux['wpcT'].ptr and (C, T, K) == (c_, 9, 4 * k_)
                f = lambda w, n=n, mode=mode: R.restate32_collapse(packed(w, n.layer.W), mode).reshape(C, 9, K)
                n_items['transpose_of_wpc'] += 1
            else:
                off = (s.ptr - st.w.ptr) // 4
                assert 0 <= off and off + C * T * K <= st.n_train and (s.ptr - st.w.ptr) % 4 == 0
                f = lambda w, off=off: w[key][off:off + C * T * K].reshape(C, T, K)
                n_items['transpose'] += 1
            got = np.empty(C * T * K, np.float32)
            plan.dev.d2h(got, t.ptr, got.nbytes)
            e0, e1, e2 = (R.transpose(f(w)).reshape(-1) for w in (w0, w1, w2))
            what = "%s %s transposed copy of [%d][%d][%d]" % (dtype, key, C, T, K)
            assert not R.bits_equal(e0, e1) and not R.bits_equal(e1, e2), (what, "the weights did not move: the test proves nothing")
            assert not R.bits_equal(got, e0), (what, "still the transform of the INITIAL weights")
            when.add('before' if R.bits_equal(got, e1) else ('after' if R.bits_equal(got, e2) else 'neither'))
            LEDGER.record('engine transpose')
            assert 'neither' not in when, (what, "the transform of no weights this run has had")
    print("engine operands %s: %s; transposed copies hold the weights %s the second step's update" % (dtype, n_items, sorted(when)))
    # every kind the mode has (fp32: no packs; bf16: every master-weight data gradient reads a transposed PACK, only a collapsed
    # layer keeps an fp32 transposed copy) is there: the walk cannot pass empty
    assert n_items['wpc'] > 0 and n_items['bias4'] > 0 and n_items['transpose_of_wpc'] > 0
    if dtype == 'f32':
        assert n_items['pack'] == 0 and n_items['pack_transposed'] == 0 and n_items['transpose'] > 0
    else:
        assert n_items['pack'] > 0 and n_items['pack_transposed'] > 0 and (n_items['transpose'] > 0) == (dtype == 'bf16x3')
    assert when == {'before'}, when
    eng.sync()
    del model
