"""Float64 definitions, inputs, row tables and bounds of the pooled block's gradient kernels -- Conv2D 5x5 'same' ->
activation -> MaxPool2D(2), whose full-resolution gradient never exists: pool_thin_wgrad_kernel + pool_thin_wgrad_final and
pool_thin_dgrad_kernel (csrc/conv_pool_bwd.hip), maxpool2_mask_bwd_compress_kernel (csrc/elementwise_q.hip) and
sp_wgrad_pooled_kernel (csrc/conv_split.hip).  Shared by tests/test_pool_bwd_ref.py (CPU: validates the reference, the inputs,
the rows' claims, measures the bound, shows what the per-element checks see) and tests/test_gpu_pool_bwd.py (GPU).  numpy
only; built on oracle/ops.py.

Definition, from the operands alone (mask [N, K, H/2, W/2] bytes, pooled gradient gp, pooled activation yp or None):
  v = gp * act'           act' from yp (dact_from_out) or, yp None, from the mask's sign bit 16 (dact_from_sign);
  G[2 i + (b >> 1), 2 j + (b & 1)] = v   for every set bit b of the low nibble: ties send v to every arg-max, nibble 0 nothing;
  dW, db, dx = oracle.ops.conv2d_vjp(x, W, G): db counts ties.
Compressed form of fine row 2 i + r (b0, b1 = bits 2 r, 2 r + 1): cq = (b0 | b1) ? v : 0 as pieces(., dtype), column bit
b1 & ~b0, flags[n * H + y] = any(b0 & b1) over the filters and columns, idx[n][cb][y][j / 16] = 8 u16 words (one per filter of
the block of 8), bit j % 16 of a word the column bit of half-pixel j.

Per-element bound:  |got - ref| <= k 2^-24 M, M the same contraction of the absolute values (+ |previous| nowhere: every
accumulate here is fl32(previous + increment)).  k = K_BOUND[family]: twice the worst of the family's fp32 restatement over its
real-input rows, rounded up; k <= n + S + 2 whatever is measured.

restate32_wgrad IS pool_thin_wgrad_kernel's order, so it is no more favourable than the kernel: lane l of a (sample, band,
filter) wave walks its items (pooled row, 64-pixel segment) in sequence and, per item, the set mask bits in ascending order,
one fmaf per tap into the tap's accumulator (the bias tap: v * popcount, fused); the 64 lanes are added by the 6-level xor
butterfly (32, 16, .., 1); pool_thin_wgrad_final's lane l then adds partials l, l + 64, .. in sequence from zero and the same
butterfly follows.  (U and KPW change which wave owns a filter and how far loads run ahead, not this order.)
restate32_dgrad is ONE sequential fmaf accumulator per pixel over the K x 9 cells (filters outermost, cells (dr, dc) row by
row, the set bits ascending) with the zero-border taps as fmaf(v, 0, o): pool_thin_dgrad_kernel's own chain o00 .. o11.
A fused multiply-add is restated as the float64 product and sum rounded once to fp32.
The split modes take tests/conv_s2_ref.py's weight-gradient reference and k (the kept piece products, K_BOUND[(mode,
'wgrad')]): no new definition.
"""
import collections

import numpy as np

from oracle import ops as O
from tests import conv_s2_ref as S2
from tests.conv_s2_ref import FRONT, _signed, hash_g, view_layout  # noqa: F401
from tests.conv_thin_ref import act64, pool_ref  # noqa: F401
from tests.elementwise_q_ref import U, dact_from_out, dact_from_sign, pieces, rel, worst  # noqa: F401

SLOPE = 0.25                        # the integer pass: exact
ALPHA = 0.2                         # the real pass: LeakyRectify(0.2)
ACTS = ('lrelu', 'relu', 'linear')
REL_L2 = 1e-5                       # tests/test_gpu_ops.py::test_conv_pool_backward_from_the_pooled_operands
MAXABS = {'bf16x3': 2e-6, 'bf16x2': 3e-5}      # max |got - ref| / max |ref|: test_pooled_weight_gradient_on_the_sparse_matrix_instruction
CUS = 256
T = 25

# ---- the frozen k per family: 2 x the worst of the restatement over the family's real-input rows (in the comment), rounded
# up; tests/test_pool_bwd_ref.py re-measures and asserts exactly that.  (db is an output of the weight-gradient family.) ----
K_BOUND = {
    'wgrad': 4,                     # 1.77  (the Wp = 1 row: sums of 16 terms; the rows with wide maps stay below 1.1)
    'dgrad': 14,                    # 6.72  (K = 64: 576 cells in one chain)
    'bf16x3': S2.K_BOUND[('bf16x3', 'wgrad')], 'bf16x2': S2.K_BOUND[('bf16x2', 'wgrad')],
}


# ---- the definition ----
def slope_of(mask, yp, act, alpha):
    return dact_from_out(yp, act, alpha) if yp is not None else dact_from_sign(mask, act, alpha)


def dense_grad(mask, yp, gp, act, alpha, dtype=np.float64):
    """G [N, K, H, W] of the definition; dtype float32: v rounded once (what a kernel that multiplies in fp32 holds)"""
    mask = np.asarray(mask)
    v = np.asarray(gp, np.float64) * slope_of(mask, yp, act, alpha)
    if dtype == np.float32:
        v = v.astype(np.float32)
    N, K, Hp, Wp = mask.shape
    G = np.zeros((N, K, 2 * Hp, 2 * Wp), dtype)
    for b in range(4):
        G[:, :, (b >> 1)::2, (b & 1)::2] = np.where((mask >> b) & 1, v, 0)
    return G


def ref(x, W, mask, yp, gp, act, alpha):
    """-> dict(dW [K, 1, 5, 5], db [K], dx [N, 1, H, W]) in float64"""
    G = dense_grad(mask, yp, gp, act, alpha)
    dx, dW, db = O.conv2d_vjp(np.asarray(x, np.float64), np.asarray(W, np.float64), G, 1, 2)
    return dict(dW=dW, db=db, dx=dx)


def magnitude(x, W, mask, yp, gp, act, alpha):
    G = np.abs(dense_grad(mask, yp, gp, act, alpha))
    dx, dW, db = O.conv2d_vjp(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64)), G, 1, 2)
    return dict(dW=dW, db=db, dx=dx)


def wgrad64(x, G):
    """the float64 5x5 'same' weight gradient [K, C, 5, 5] of any channel count (the split rows)"""
    x, G = np.asarray(x, np.float64), np.asarray(G, np.float64)
    return O.conv2d_vjp(x, np.zeros((G.shape[1], x.shape[1], 5, 5)), G, 1, 2)[1]


def ref_split(mode, x, G32):
    """conv_s2_ref.ref_mode for the 5x5 product: fp32 operands ('bf16x3'), the three kept piece products ('bf16x2')"""
    if mode == 'bf16x3':
        return wgrad64(x, G32)
    return sum(wgrad64(a, b) for a, b in S2.piece_pairs(mode, x, G32))


def compressed(mask, yp, gp, act, alpha, dtype):
    """-> (cq pieces: tuple of float32 [N, K, H, W / 2], idx uint16 [N, K / 8, H, W / 32, 8], flags int32 [N * H])"""
    mask = np.asarray(mask)
    N, K, Hp, Wp = mask.shape
    v = (np.asarray(gp, np.float64) * slope_of(mask, yp, act, alpha)).astype(np.float32)
    cq = np.zeros((N, K, 2 * Hp, Wp), np.float32)
    col = np.zeros((N, K, 2 * Hp, Wp), np.uint16)
    tie = np.zeros((N, K, 2 * Hp, Wp), bool)
    for r in range(2):
        b0, b1 = (mask >> (2 * r)) & 1, (mask >> (2 * r + 1)) & 1
        cq[:, :, r::2] = np.where(b0 | b1, v, np.float32(0))
        col[:, :, r::2] = b1 & ~b0 & 1
        tie[:, :, r::2] = (b0 & b1) != 0
    flags = tie.any(axis=(1, 3)).astype(np.int32).reshape(N * 2 * Hp)
    w = (col.reshape(N, K // 8, 8, 2 * Hp, Wp // 16, 16) << np.arange(16, dtype=np.uint16)).sum(-1).astype(np.uint16)
    return pieces(cq, dtype), np.ascontiguousarray(w.transpose(0, 1, 3, 4, 2)), flags


# ---- fp32 restatements ----
def _fma(a, b, c):
    return (a.astype(np.float64) * b + c).astype(np.float32)


def _butterfly(s):
    """the xor butterfly over axis -2 (64 lanes): every lane ends with the same bits; lane 0's"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[..., lanes ^ off, :]).astype(np.float32)
    return s[..., 0, :]


def wgrad_ldp(W):
    return (W // 2 + 2 + 63) // 64 * 64


def wgrad_rb(H, W):
    for rb in (8, 4, 2, 1):
        if (H // 2) % rb == 0 and (2 * rb + 4) * 2 * wgrad_ldp(W) * 4 <= 52 * 1024:
            return rb
    return 0


def restate32_wgrad(x, mask, yp, gp, act, alpha):
    """-> (dW [K, 1, 5, 5], db [K]) in the kernels' own order (module docstring)"""
    x, mask = np.asarray(x, np.float32), np.asarray(mask)
    N, K, Hp, Wp = mask.shape
    rb = wgrad_rb(2 * Hp, 2 * Wp)
    bands, nseg = Hp // rb, (Wp + 63) // 64
    v = (np.asarray(gp, np.float32) * slope_of(mask, None if yp is None else np.asarray(yp, np.float32), act, np.float32(alpha)).astype(np.float32)).astype(np.float32)
    xp = np.pad(x[:, 0], ((0, 0), (2, 2), (2, 2 + 2 * 64)))
    acc = np.zeros((N, bands, K, 64, T + 1), np.float32)
    lane, ar = np.arange(64), np.arange(5)
    for r in range(rb):
        rows = np.arange(bands) * rb + r                                            # pooled row of every band
        for s in range(nseg):
            px = s * 64 + lane
            ok = px < Wp
            pxc = np.minimum(px, Wp - 1)
            vv = np.where(ok, v[:, :, rows][..., pxc], np.float32(0)).transpose(0, 2, 1, 3)        # [N, bands, K, 64]
            mm = np.where(ok, mask[:, :, rows][..., pxc] & 15, 0).transpose(0, 2, 1, 3)
            pop = sum((mm >> b) & 1 for b in range(4)).astype(np.float32)
            acc[..., T] = _fma(vv, pop, acc[..., T])
            for b in range(4):
                by, bx = b >> 1, b & 1
                yy = (2 * rows + by)[:, None, None, None] + ar[None, None, :, None]                 # [bands, 1, 5, 1]
                xx = (2 * px + bx)[None, :, None, None] + ar[None, None, None, :]                   # [1, 64, 1, 5]
                win = xp[:, yy, xx].reshape(N, bands, 1, 64, T)                                     # x[ay + ta - 2][ax + tb - 2]
                on = ((mm >> b) & 1).astype(bool)[..., None]
                acc[..., :T] = np.where(on, _fma(vv[..., None], win, acc[..., :T]), acc[..., :T])
    part = _butterfly(acc).reshape(N * bands, K, T + 1)                                             # [S, K, 26]
    S = part.shape[0]
    lanes = np.zeros((K, 64, T + 1), np.float32)
    for s0 in range(0, S, 64):
        chunk = part[s0:s0 + 64]
        lanes[:, :len(chunk)] = (lanes[:, :len(chunk)] + chunk.transpose(1, 0, 2)).astype(np.float32)
    out = _butterfly(lanes)                                                                          # [K, 26]
    # tap (ta, tb) of the correlation = packed tap t: dW[k, 0, 4 - ta, 4 - tb]
    return np.ascontiguousarray(out[:, :T].reshape(K, 1, 5, 5)[:, :, ::-1, ::-1]), out[:, T].copy()


def restate32_dgrad(W, mask, yp, gp, act, alpha, drop=None):
    """-> dx [N, 1, H, W]: one sequential accumulator per pixel.  ``drop`` = (cy, cx, dr, dc): that thread skips that
    neighbour cell (the halo mutation of tests/test_pool_bwd_ref.py)"""
    mask = np.asarray(mask)
    N, K, Hp, Wp = mask.shape
    Wc = np.asarray(W, np.float32)[:, 0, ::-1, ::-1]                                # Wc[k][ta][tb], the packed order
    Wl = np.zeros((K, 7, 8), np.float32)
    Wl[:, 1:6, 1:6] = Wc
    v = (np.asarray(gp, np.float32) * slope_of(mask, None if yp is None else np.asarray(yp, np.float32), act, np.float32(alpha)).astype(np.float32)).astype(np.float32)
    vp = np.pad(v, ((0, 0), (0, 0), (1, 1), (1, 1)))
    mp = np.pad(mask & 15, ((0, 0), (0, 0), (1, 1), (1, 1)))
    o = np.zeros((N, Hp, 2, Wp, 2), np.float32)
    for k in range(K):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                vv = vp[:, k, 1 + dr:1 + dr + Hp, 1 + dc:1 + dc + Wp]
                mm = mp[:, k, 1 + dr:1 + dr + Hp, 1 + dc:1 + dc + Wp].copy()
                if drop is not None and (dr, dc) == tuple(drop[2:]):
                    mm[:, drop[0], drop[1]] = 0
                for b in range(4):
                    on = ((mm >> b) & 1).astype(bool)
                    r0, c0 = (3 - 2 * dr) - (b >> 1), (3 - 2 * dc) - (b & 1)
                    for pr in range(2):
                        for pc in range(2):
                            o[:, :, pr, :, pc] = np.where(on, _fma(vv, Wl[k, r0 + pr, c0 + pc], o[:, :, pr, :, pc]), o[:, :, pr, :, pc])
    return o.reshape(N, 1, 2 * Hp, 2 * Wp)


# ---- inputs ----
def make_mask(shape_p, row_seams, col_seams, seed, forward=None):
    """the low nibbles [N, K, Hp, Wp] of a row's mask: random nibbles with every tie order and nibble 0, every one of the four
    arg-max positions on both sides of every border and seam (pooled rows / columns in ``row_seams`` / ``col_seams``, each with
    its predecessor), two- and four-way ties on the first and last pooled row and column, and one whole tied plane (the last
    sample's last filter; none when N K = 1).  ``forward``: nibbles of a forward pass to start from instead of random ones"""
    N, K, Hp, Wp = shape_p
    r = np.random.RandomState(seed % (2 ** 31))
    if forward is not None:
        m = (np.asarray(forward) & 15).astype(np.uint8)
    else:
        m = (1 << r.randint(0, 4, shape_p)).astype(np.uint8)
        other = r.randint(0, 16, shape_p).astype(np.uint8)
        m = np.where(r.rand(*shape_p) < 0.3, other, m).astype(np.uint8)
    rows = sorted({p for s in list(row_seams) + [0, Hp] for p in (s - 1, s) if 0 <= p < Hp})
    cols = sorted({p for s in list(col_seams) + [0, Wp] for p in (s - 1, s) if 0 <= p < Wp})
    inner = np.ones((Hp, Wp), bool)
    inner[rows], inner[:, cols] = False, False
    spots = np.argwhere(inner)
    if len(spots) >= 16:            # every nibble once, away from the seams, in the first plane
        pick = spots[r.permutation(len(spots))[:16]]
        m[0, 0, pick[:, 0], pick[:, 1]] = np.arange(16, dtype=np.uint8)
    plane = np.arange(N)[:, None, None] + np.arange(K)[None, :, None]          # (the position also turns with the plane)
    for q, i in enumerate(rows):
        m[:, :, i, :] = 1 << ((np.arange(Wp)[None, None] + plane + q) % 4)
    for q, j in enumerate(cols):
        m[:, :, :, j] = 1 << ((np.arange(Hp)[None, None] + plane + q + 1) % 4)
    for i, j in ((0, slice(0, None, 7)), (Hp - 1, slice(3, None, 7))):
        m[:, 0::2, i, j], m[:, 1::2, i, j] = 3, 15
    for j, i in ((0, slice(1, None, 5)), (Wp - 1, slice(2, None, 5))):
        m[:, 0::2, i, j], m[:, 1::2, i, j] = 12, 15
    # three-bit windows and empty ones on the borders too (a map of one or two pooled rows has nothing but borders)
    m[:, 0::2, 0, 5::11], m[:, 1::2, 0, 5::11], m[:, 0::2, Hp - 1, 8::13], m[:, 1::2, Hp - 1, 8::13] = 7, 0, 0, 14
    m[:, 0::2, 3::11, 0], m[:, 1::2, 3::11, 0], m[:, 0::2, 4::13, Wp - 1], m[:, 1::2, 4::13, Wp - 1] = 13, 0, 0, 11
    if N * K > 1:
        m[N - 1, K - 1] = 15
    return m


def with_sign(nib, yp):
    return ((np.asarray(nib) & 15) | ((np.asarray(yp) > 0).astype(np.uint8) << 4)).astype(np.uint8)


def _yp(r, shape_p, integer):
    """positives, negatives and exact zeros"""
    yp = r.randint(-2, 3, shape_p).astype(np.float32) if integer else r.randn(*shape_p).astype(np.float32)
    if not integer:
        yp[r.rand(*shape_p) < 0.1] = 0.0
    return yp


def inputs(g, seams, integer, C=1, salt=0):
    """g = (N, H, W, K) -> dict(x, W, gp, yp, mask, prev_dW, prev_db, prev_dx).  Integer: x, gp in +-{1, 2, 3}, W in +-{1, 2},
    yp in -2 .. 2: exact in bf16, the second and third split pieces zero.  Real: the scaled draws of tests/conv_s2_ref.py"""
    N, H, Wd, K = g
    sp = (N, K, H // 2, Wd // 2)
    r = np.random.RandomState((hash_g(g) + 7 * C + salt + (0 if integer else 1000)) % (2 ** 31))
    if integer:
        d = dict(x=_signed(r, 3, (N, C, H, Wd)), W=_signed(r, 2, (K, C, 5, 5)), gp=_signed(r, 3, sp),
                 prev_dW=_signed(r, 7, (K, C, 5, 5)), prev_db=_signed(r, 7, (K,)), prev_dx=_signed(r, 7, (N, C, H, Wd)))
    else:
        d = dict(x=(r.randn(N, C, H, Wd) * np.exp(r.randn(N, C, 1, 1))).astype(np.float32),
                 W=(r.randn(K, C, 5, 5) / np.sqrt(25.0 * C)).astype(np.float32),
                 gp=(r.randn(*sp) * np.exp(r.randn(N, K, 1, 1))).astype(np.float32),
                 prev_dW=r.randn(K, C, 5, 5).astype(np.float32), prev_db=r.randn(K).astype(np.float32),
                 prev_dx=r.randn(N, C, H, Wd).astype(np.float32))
    d['yp'] = _yp(r, sp, integer)
    d['mask'] = with_sign(make_mask(sp, seams[0], seams[1], hash_g(g) + 3 + salt), d['yp'])
    return d


def forward_inputs(g, integer, salt=0):
    """the same with mask and yp from a float64 forward conv -> bias -> lrelu rounded to fp32 -> max-pool (constant patches in x:
    tied windows), C = 1"""
    d = inputs(g, ((), ()), integer, salt=salt)
    N, H, Wd, K = g
    x = d['x'].copy()
    x[:, :, :max(H // 4, 2), :max(Wd // 4, 2)] = 1.0 if integer else 0.25
    x[-1] = 0.0
    r = np.random.RandomState((hash_g(g) + 99) % (2 ** 31))
    b = _signed(r, 2, (K,)) if integer else r.randn(K).astype(np.float32)
    y = act64(O.conv2d_fwd(x.astype(np.float64), d['W'].astype(np.float64), b.astype(np.float64), 1, 2), 'lrelu')
    yp, mask = pool_ref(y.astype(np.float32))
    d.update(x=x, yp=yp.astype(np.float32), mask=mask)
    return d


# ---- the row tables ----
Row = collections.namedtuple('Row', 'g view reaches why')


def _w(g, view, rb, why):
    N, H, W, K = g
    return Row(g, view, dict(rb=rb, nseg=(W // 2 + 63) // 64, items=rb * ((W // 2 + 63) // 64), S=N * (H // 2) // rb), why)


# sparse fp32 weight gradient, (N, H, W, K); reaches: rb, nseg, items = rb nseg, S = N bands
WGRAD_ROWS = [
    _w((2, 16, 32, 8), 'whole', 8, "rb 8 by divisibility (Hp 8); one filter per wave"),
    _w((2, 8, 32, 9), 'slice', 4, "rb 4 (Hp 4); K 9: the second KPW round holds one live wave"),
    _w((1, 12, 32, 16), 'offset', 2, "rb 2 (Hp 6); K 16 fills one block; items 2 < U"),
    _w((1, 46, 32, 17), 'whole', 1, "rb 1 (Hp 23); K 17: a second blockIdx.z with one filter; items 1"),
    _w((2, 16, 636, 1), 'slice', 8, "the widest rb 8 (52 KB rule); K 1: seven idle waves; nseg 5, items 40"),
    _w((1, 16, 638, 8), 'whole', 4, "one column pair wider: rb falls to 4 at Hp 8"),
    _w((1, 16, 1024, 8), 'offset', 2, "W 1024, Hp 8: rb 2"),
    _w((1, 2, 2172, 8), 'whole', 1, "the last served width; nseg 17: items 17, no multiple of U"),
    _w((2, 16, 2, 8), 'offset', 8, "Wp 1: one live lane per segment"),
    _w((1, 8, 126, 64), 'slice', 4, "Wp 63: the px < Wp tail; K 64: four blockIdx.z"),
    _w((1, 4, 128, 65), 'whole', 2, "Wp 64: one full segment; K 65: a fifth blockIdx.z with one filter"),
    _w((1, 6, 130, 96), 'offset', 1, "Wp 65: a second segment with one live lane; K 96; items 2 < U"),
    _w((1, 4, 262, 8), 'slice', 2, "Wp 131, nseg 3: items 6, above U and no multiple of it"),
    _w((64, 2, 8, 8), 'whole', 1, "S = 64: every lane of the final kernel adds exactly one partial"),
    _w((3, 46, 16, 8), 'slice', 1, "S = 69 (N 3, 23 bands): lanes 0 .. 4 add two partials"),
]
WGRAD_FORWARD = [(2, 16, 32, 8), (2, 8, 32, 9)]        # rows run a second time with mask and yp from a forward pass
WGRAD_UNSERVED = (1, 2, 2174, 8)                          # bit 0 clear


def _d(g, view, why):
    N, H, W, K = g
    return Row(g, view, dict(tiles=((H // 2 + 7) // 8, (W // 2 + 31) // 32), rounds=(K + 7) // 8, kn=K - (K - 1) // 8 * 8), why)


# sparse fp32 data gradient, (N, H, W, K); reaches: (tile rows, tile columns), KC rounds, kn of the last round
DGRAD_ROWS = [
    _d((2, 2, 2, 1), 'whole', "Hp 1, Wp 1, K 1: one live thread, kn 1"),
    _d((1, 16, 64, 8), 'slice', "Hp 8, Wp 32: exactly one cell tile, one full round"),
    _d((2, 18, 66, 9), 'offset', "Hp 9, Wp 33: 2 x 2 tiles with one live row / column in the far ones; K 9: a round with kn 1"),
    _d((1, 18, 64, 64), 'whole', "K 64: eight rounds, the whole filter LDS"),
    _d((1, 2, 66, 8), 'slice', "Hp 1 with a tile seam in the columns"),
    _d((3, 16, 2, 8), 'offset', "Wp 1, Hp 8"),
]
DGRAD_FORWARD = [(2, 18, 66, 9)]
DGRAD_REFUSED_K = (1, 16, 64, 65)


def wgrad_seams(g):
    N, H, W, K = g
    rb = wgrad_rb(H, W) or 1
    return range(rb, H // 2, rb), range(64, W // 2, 64)


def dgrad_seams(g):
    N, H, W, K = g
    return range(8, H // 2, 8), range(32, W // 2, 32)


# compress + sparse-instruction weight gradient, (N, C, K, H, W); reaches: strip width, row splits per strip, rows per split
SplitRow = collections.namedtuple('SplitRow', 'g env reaches why')
ROUNDS2 = {'GHM_SPLIT_WGRAD_ROUNDS': '0.02'}
SPLIT_ROWS = [
    SplitRow((1, 32, 64, 2, 32), {}, dict(spx=32, splits=1, rows=2, hwp=16), "one pooled row, 32-pixel strips, hwp 16 < 256"),
    SplitRow((2, 32, 64, 16, 64), ROUNDS2, dict(spx=64, splits=2, rows=8, hwp=256), "64-pixel strips, two row splits"),
    SplitRow((1, 64, 128, 4, 96), {}, dict(spx=32, splits=1, rows=4, hwp=96), "three strips, two channel groups, two filter-tile rows"),
    SplitRow((3, 32, 64, 6, 128), {}, dict(spx=64, splits=1, rows=6, hwp=192), "three samples, two 64-pixel strips"),
    SplitRow((1, 32, 64, 18, 64), {}, dict(spx=64, splits=2, rows=9, hwp=288), "hwp 288: a partly live second compress block; splits of 9 rows cut a window"),
]
SPLIT_MODES = ('bf16x3', 'bf16x2')
FLAG_PATTERNS = ('none', 'all', 'alternate', 'first', 'last')


def split_plan(g, env=None, cus=CUS):
    """sp_wplan's 5x5 branch restated -> dict(spx, splits, rows) (the strip width and split count show in no query; the
    workspace bytes, which do, are N strips x splits x C 25 K floats: tests/test_pool_bwd_ref.py holds the two together)"""
    N, C, K, H, W = g
    spx = 64 if W % 64 == 0 else 32
    ncols = N * (W // spx)
    tiles = (C // 32) * (K // 64) * ncols
    S = cus // tiles
    if env and 'GHM_SPLIT_WGRAD_ROUNDS' in env:
        S = int(float(env['GHM_SPLIT_WGRAD_ROUNDS']) * cus / tiles)
    S = max(min(S, max(H // 8, 1)), 1)
    rows = (H + S - 1) // S
    return dict(spx=spx, splits=(H + rows - 1) // rows, rows=rows)


def flagged_rows(g, plan, pattern):
    """the fine rows (of every sample) that hold a tied window row"""
    H, rows = g[3], plan['rows']
    starts = list(range(0, H, rows))
    return {'none': [], 'all': list(range(H)), 'alternate': list(range(0, H, 2)), 'first': starts,
            'last': [min(s + rows, H) - 1 for s in starts]}[pattern]


def split_inputs(g, plan, pattern, integer):
    """x [N, C, H, W], gp, yp, mask for a split row: nibbles without a tied window row (one bit, or one bit in each row: 5, 6,
    9, 10, and nibble 0) except in the fine rows of ``pattern``, which get two-bit row ties (and whole tied windows where
    both rows of a window are flagged) in a few filters and columns"""
    N, C, K, H, W = g
    d = inputs((N, H, W, K), ((), ()), integer, C=C, salt=11)
    r = np.random.RandomState((hash_g(g) + 31) % (2 ** 31))
    sp = (N, K, H // 2, W // 2)
    free = np.array([1, 2, 4, 8, 5, 6, 9, 10, 0, 1, 2, 4, 8], np.uint8)
    m = free[r.randint(0, len(free), sp)]
    fl = set(flagged_rows(g, plan, pattern))
    for y in sorted(fl):
        i, rr = y // 2, y % 2
        ks, js = slice(y % 3, None, 3), slice(y % 5, None, 5)
        m[:, ks, i, js] = (m[:, ks, i, js] & (12 if rr == 0 else 3)) | (3 if rr == 0 else 12)
        m[:, 0, i, 0] = (m[:, 0, i, 0] & (12 if rr == 0 else 3)) | (3 if rr == 0 else 12)       # (the first column, always)
    d['mask'] = with_sign(m, d['yp'])
    return d


def row_id(r):
    return "x".join(str(v) for v in r.g) + ("-" + r.view if hasattr(r, 'view') else "")


def border_class(name, shape, index):
    if name == 'dx':
        edge = lambda v, n: "first" if v == 0 else ("last" if v == n - 1 else "inner")
        return "sample %d, %s row, %s column, cell tile (%d, %d)" % (index[0], edge(index[2], shape[2]), edge(index[3], shape[3]), index[2] // 16, index[3] // 64)
    if name == 'db':
        return "bias of filter %d" % index[0]
    return "tap (%d, %d) of filter %d, channel %d" % (index[2], index[3], index[0], index[1])
