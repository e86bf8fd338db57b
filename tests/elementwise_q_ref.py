"""Float64 definitions of the element-wise q producers (csrc/elementwise_q.hip) and of their two neighbours in
csrc/elementwise.hip, the expected stored halfwords of a q tensor in the four dtypes, canary helpers, and the shape tables
and input sets of tests/test_gpu_elementwise_q.py (shared with tests/test_elementwise_q_ref.py, which validates the inputs
and the bounds on the CPU).  numpy only; built on oracle/ops.py where the op exists there.

Per-element bound of every op:  |got - ref| <= k * 2^-24 * M.
  M  float64 sum of the absolute values of the terms of the element's expression (returned beside the value),
  k  number of fp32 roundings in the kernel's expression plus one, counted from the source and stated in K_* below.
Every ``restate32_*`` function is the kernel's expression in float32 numpy (a fused multiply-add as the float64 product
and sum rounded once): the CPU module proves that plain fp32 arithmetic stays inside the bound on every input set.
"""
import numpy as np

from oracle import lp as LP
from oracle import ops as O

U = 2.0 ** -24                      # unit roundoff of fp32
ALPHA = 0.2                         # LeakyRectify(0.2); the kernels receive it as a float
ACTS = ('lrelu', 'relu', 'linear')
DTYPES = ('bf16', 'f16', 'bf16x3', 'bf16x2')
PLANES = {'bf16': 1, 'f16': 1, 'bf16x3': 3, 'bf16x2': 2}
CANARY = 0x7fc1                     # a NaN as bf16, as fp16 and (twice) as fp32: no kernel here produces it from finite inputs

# ---- k per op (roundings + 1) ----
# bn_apply_q_kernel / bn_apply_hi_kernel: act(fmaf(x - m, gamma * inv, beta)): gamma * inv, x - m, the fma = 3; leaky relu
# multiplies once more; tanhf is specified to 2 ulp = 4 unit roundoffs (all four activations are 1-Lipschitz, so the error of
# the pre-activation passes through unamplified)
K_BN_APPLY = {'linear': 4, 'relu': 4, 'lrelu': 5, 'tanh': 8}
# bn_bwd_apply_q_kernel / bn_bwd_hi_apply: g * (d * act' - mb - (x - m) * iv * mg): g = gamma * iv (1), d * act' (1),
# mb = float(sum) * (1.f / count): 3, the subtraction (1), x - m (1), * iv (1), mg (3), * mg (1), the subtraction (1), * g (1) = 14
K_BN_BWD = 15
K_BILINEAR = 4                      # a11 = 0.5 * (0.5 * (v00 + v10) + 0.5 * (v01 + v11)): three sums (halving is exact)
K_INTERLEAVE = 1                    # a copy
K_MASK_BWD = 2                      # dy * act'(y): one product
REL_L2 = 1e-5                       # the per-op bound of tests/test_gpu_ops.py


def a32(alpha):
    return float(np.float32(alpha))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


def worst(got, ref, M):
    """max over the elements of |got - ref| / (2^-24 M), in units of k (0 where got == ref)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / (U * np.asarray(M, np.float64)))
    return float(r.max()) if r.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- activations ----
def act_fwd(v, act, alpha=0.0):
    v = np.asarray(v, np.float64)
    if act == 'relu':
        return O.relu_fwd(v)
    if act == 'lrelu':
        return np.where(v > 0, v, a32(alpha) * v)
    if act == 'sigmoid':
        return O.sigmoid_fwd(v)
    if act == 'tanh':
        return O.tanh_fwd(v)
    assert act == 'linear'
    return v


def dact_from_out(y, act, alpha=0.0):
    """act'(.) as a function of the OUTPUT y (slope ``alpha`` at y <= 0 for the leaky relu: DESIGN, measure-zero differences)"""
    y = np.asarray(y, np.float64)
    if act == 'relu':
        return (y > 0).astype(np.float64)
    if act == 'lrelu':
        return np.where(y > 0, 1.0, a32(alpha))
    if act == 'sigmoid':
        return y * (1 - y)
    if act == 'tanh':
        return 1 - y * y
    assert act == 'linear'
    return np.ones_like(y)


def dact_from_sign(mask, act, alpha=0.0):
    """the same slope from bit 4 of a pooling mask byte (set where the pooled activation is > 0)"""
    pos = (np.asarray(mask) & 16) != 0
    if act == 'linear':
        return np.ones(pos.shape)
    return np.where(pos, 1.0, 0.0 if act == 'relu' else a32(alpha))


def restate32_act(v32, act, alpha=0.0):
    v32 = np.asarray(v32, np.float32)
    if act == 'relu':
        return np.where(v32 > 0, v32, np.float32(0))
    if act == 'lrelu':
        return np.where(v32 > 0, v32, np.float32(alpha) * v32).astype(np.float32)
    if act == 'tanh':
        return np.tanh(v32.astype(np.float64)).astype(np.float32)
    if act == 'sigmoid':
        return (np.float32(1) / (np.float32(1) + np.exp(-v32.astype(np.float64)).astype(np.float32))).astype(np.float32)
    return v32


def restate32_dact(y32, act, alpha=0.0):
    y32 = np.asarray(y32, np.float32)
    if act == 'relu':
        return (y32 > 0).astype(np.float32)
    if act == 'lrelu':
        return np.where(y32 > 0, np.float32(1), np.float32(alpha)).astype(np.float32)
    if act == 'sigmoid':
        return (y32 * (np.float32(1) - y32)).astype(np.float32)
    if act == 'tanh':
        return (np.float32(1) - y32 * y32).astype(np.float32)
    return np.ones_like(y32)


# ---- BatchNorm ----
def _sh(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def bn_stats(x):
    """batch statistics of oracle.ops.bn_train_fwd in float64, as the float32 vectors the kernels are given"""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    _, mu, inv = O.bn_train_fwd(x, np.zeros(C), np.ones(C))
    return mu.astype(np.float32), inv.astype(np.float32)


def bn_apply(x, mean, inv, gamma, beta, act, alpha=0.0):
    """-> (y, M): act((x - mean) * (gamma * inv) + beta) of the float32 inputs, in float64"""
    t, sc = np.asarray(x, np.float64) - _sh(mean), _sh(gamma) * _sh(inv)
    return act_fwd(t * sc + _sh(beta), act, alpha), np.abs(t * sc) + np.abs(_sh(beta))


def restate32_bn_apply(x, mean, inv, gamma, beta, act, alpha=0.0):
    s = lambda v: np.asarray(v, np.float32).reshape(1, -1, 1, 1)
    sc = s(gamma) * s(inv)
    t = np.asarray(x, np.float32) - s(mean)
    pre = (t.astype(np.float64) * sc + s(beta)).astype(np.float32)
    return restate32_act(pre, act, alpha)


def bn_backward(dout, y, x, mean, inv, gamma, act, alpha=0.0):
    """-> (dx, M, dgamma, dbeta) of oracle.ops.bn_train_vjp with dz = dout * act'(y) in front, in float64; y is the layer's
    float32 output (the kernels that are given no y recompute exactly that tensor from x)"""
    dz = np.asarray(dout, np.float64) * dact_from_out(y, act, alpha)
    xh = (np.asarray(x, np.float64) - _sh(mean)) * _sh(inv)
    dbeta, dgamma = dz.sum(axis=(0, 2, 3)), (dz * xh).sum(axis=(0, 2, 3))
    cnt = dz.size // dz.shape[1]
    mb, mg, g = _sh(dbeta / cnt), _sh(dgamma / cnt), _sh(gamma) * _sh(inv)
    return g * (dz - mb - xh * mg), np.abs(g) * (np.abs(dz) + np.abs(mb) + np.abs(xh * mg)), dgamma, dbeta


def restate32_bn_backward(dout, y, x, mean, inv, gamma, act, alpha=0.0):
    s = lambda v: np.asarray(v, np.float32).reshape(1, -1, 1, 1)
    dz = (np.asarray(dout, np.float32) * restate32_dact(y, act, alpha)).astype(np.float32)
    xh = ((np.asarray(x, np.float32) - s(mean)) * s(inv)).astype(np.float32)
    sa = dz.astype(np.float64).sum(axis=(0, 2, 3)).astype(np.float32)               # fp64 sums, rounded once
    sb = (dz.astype(np.float64) * xh).sum(axis=(0, 2, 3)).astype(np.float32)
    ic = np.float32(1) / np.float32(dz.size // dz.shape[1])
    g, mb, mg = s(gamma) * s(inv), s(sa * ic), s(sb * ic)
    return (g * ((dz - mb) - xh * mg)).astype(np.float32)


# ---- Theano bilinear x2 ----
def bilinear(x):
    """-> (y, M): theano's bilinear_upsampling(ratio=2) transcribed (oracle.ops.bilinear_theano_literal)"""
    x = np.asarray(x, np.float64)
    return O.bilinear_theano_literal(x), O.bilinear_up2_fwd(np.abs(x))


def restate32_bilinear(x):
    return O.bilinear_up2_fwd(np.asarray(x, np.float32))        # rows first, then columns: the kernel's order


# ---- parity interleave: pp sample 4 n + p, p = 2 dy + dx, goes to hi[n, :, 2 y + dy, 2 x + dx] ----
def pp_to_hi(pp):
    N4, K, H, W = pp.shape
    return np.ascontiguousarray(pp.reshape(N4 // 4, 2, 2, K, H, W).transpose(0, 3, 4, 1, 5, 2)).reshape(N4 // 4, K, 2 * H, 2 * W)


def hi_to_pp(hi):
    N, K, H2, W2 = hi.shape
    return np.ascontiguousarray(hi.reshape(N, K, H2 // 2, 2, W2 // 2, 2).transpose(0, 3, 5, 1, 2, 4)).reshape(4 * N, K, H2 // 2, W2 // 2)


def bn_apply_hi(x_pp, mean, inv, gamma, beta, act, alpha=0.0):
    """BatchNorm + activation of a parity-planar tensor, interleaved -> (hi, M)"""
    y, M = bn_apply(x_pp, mean, inv, gamma, beta, act, alpha)
    return pp_to_hi(y), pp_to_hi(M)


def bn_backward_hi(dhi, y_pp, x_pp, mean, inv, gamma, act, alpha=0.0):
    """its backward from the interleaved gradient -> parity-planar (dx, M), dgamma, dbeta"""
    return bn_backward(hi_to_pp(np.asarray(dhi)), y_pp, x_pp, mean, inv, gamma, act, alpha)


# ---- backward of conv + act + 2x2 max-pool from the pooling mask ----
def mask_bwd(mask, y, dy, act, alpha=0.0):
    """dx[2i+dr, 2j+dc] = bit(2 dr + dc) ? dy[i, j] * act'(.) : 0, the slope from y or (y None) from mask bit 4
    -> (dx, M, dbias): dbias, the conv's bias gradient, is dx's per-channel sum"""
    mask = np.asarray(mask)
    da = dact_from_out(y, act, alpha) if y is not None else dact_from_sign(mask, act, alpha)
    g = np.asarray(dy, np.float64) * da
    N, C, Ho, Wo = mask.shape
    bit = np.stack([(mask >> b) & 1 for b in range(4)], -1).reshape(N, C, Ho, Wo, 2, 2).astype(bool)    # [dr][dc]
    dx = np.where(bit, g[..., None, None], 0.0).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return dx, np.abs(dx), dx.sum(axis=(0, 2, 3))


def restate32_mask_bwd(mask, y, dy, act, alpha=0.0):
    mask = np.asarray(mask)
    da = restate32_dact(y, act, alpha) if y is not None else dact_from_sign(mask, act, np.float32(alpha)).astype(np.float32)
    g = (np.asarray(dy, np.float32) * da).astype(np.float32)
    N, C, Ho, Wo = mask.shape
    bit = np.stack([(mask >> b) & 1 for b in range(4)], -1).reshape(N, C, Ho, Wo, 2, 2).astype(bool)
    return np.where(bit, g[..., None, None], np.float32(0)).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)


# ---- the stored halfwords ----
def pieces(a, dtype):
    """the values of the halfwords a q producer stores for the float32 array ``a``: a tuple of PLANES[dtype] float32 arrays"""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == 'bf16':
        return (LP.round_bf16(a),)
    if dtype == 'f16':
        return (LP.round_f16(a),)
    if dtype == 'bf16x3':
        return tuple(LP.split_bf16x3(a))
    assert dtype == 'bf16x2'
    return tuple(LP.split_bf16x2(a))


# ---- canaries ----
def canary_fill(dev, ptr, nbytes):
    assert nbytes % 2 == 0
    dev.h2d(ptr, np.full(nbytes // 2, CANARY, np.uint16))


def canary_changed(dev, ptr, nbytes, inside):
    """halfword indices of [ptr, ptr + nbytes) OUTSIDE the boolean halfword mask ``inside`` that no longer hold the canary"""
    raw = np.empty(nbytes // 2, np.uint16)
    dev.d2h(raw, ptr, nbytes)
    return np.flatnonzero((raw != CANARY) & ~inside)


def q_inside(planes, N, nstride, pstride, unit0, units, total_units):
    """halfword mask of a q view: ``units`` units from ``unit0`` in every sample (nstride apart) of every plane (pstride apart)"""
    m = np.zeros((total_units, 8), bool)
    for p in range(planes):
        for n in range(N):
            lo = p * pstride + n * nstride + unit0
            m[lo:lo + units] = True
    return m.reshape(-1)


def f32_inside(N, nstride, el0, els, total):
    """halfword mask of an fp32 view: ``els`` elements from ``el0`` in every sample"""
    m = np.zeros((total, 2), bool)
    for n in range(N):
        m[n * nstride + el0:n * nstride + el0 + els] = True
    return m.reshape(-1)


# ---- which branch a geometry reaches (the dispatch code of csrc/elementwise.hip / elementwise_q.hip restated) ----
BN_MAX_SPLIT = 64


def bn_sums_dispatch(N, C, HW, aligned=True):
    """ghm_bn_backward_sums -> ('rows', S) for bn_rows_partial<true>, ('flat', S) for bn_bwd_partial"""
    if aligned and HW % 4 == 0 and N <= BN_MAX_SPLIT:
        segs = min((2048 + C * N - 1) // (C * N), BN_MAX_SPLIT // N, max(HW // 2048, 1))
        segs = max(segs, 1)
        ln = ((HW + segs - 1) // segs + 3) // 4 * 4
        return 'rows', N * ((HW + ln - 1) // ln)
    S = min((1024 + C - 1) // C, max(N * HW // 2048, 1), BN_MAX_SPLIT)
    return 'flat', max(S, 1)


def bn_hi_split(N, K, H, W):
    """ghm_bn_backward_hi -> (S, chunk sizes of bn_bwd_hi_partial)"""
    count = N * H * W
    S = max(min((2048 + K - 1) // K, count // 512, BN_MAX_SPLIT), 1)
    chunk = (count + S - 1) // S
    return S, [min(chunk, count - s * chunk) for s in range(S)]


def pool_bpp(H, W, windows):
    """ghm_maxpool2_mask_bwd_q -> (items per (sample, channel block), blocks of 256 for them)"""
    items = (H // 2) * (W // 4 if windows else W)
    return items, (items + 255) // 256


# ---- the shape tables: every row names what it reaches ----
# ghm_bn_apply_q / ghm_bn_backward_q, (N, C, H, W)
BN_ROWS = [
    ((3, 24, 10, 12), "the shape of the older test; 1080 threads: the tail of q_decode; sums: rows, S = 3"),
    ((3, 8, 1, 2), "one channel block, HW = 2: the smallest legal BatchNorm map (three samples: with one, dx is pure cancellation)"),
    ((1, 16, 5, 6), "one sample; HW % 4 == 2: bn_bwd_partial (S = 1) in place of bn_rows_partial<true>; PX = 2 rows 8-byte aligned only"),
    ((2, 8, 3, 10), "HW % 4 == 2 with a single channel block"),
    ((2, 16, 64, 64), "N HW >= 4096, HW % 4 == 0: bn_rows_partial<true> with S = 4"),
    ((2, 16, 45, 46), "HW = 2070, HW % 4 == 2: bn_bwd_partial with S = 2 (chunks of 2070)"),
    ((2, 64, 128, 128), "net-sized: more than 2^16 units per plane; sums: rows, S = 16"),
]
BIG = 2 ** 18          # rows with more elements than this run one activation only
# ghm_upsample_bilinear2_fwd_q / ghm_pp_to_hi_q / ghm_bn_apply_hi, (N, C, H, W) of the COARSE map
COARSE_ROWS = [
    ((2, 8, 1, 1), "1x1: i1 == i, j1 == j; one channel block"),
    ((2, 16, 1, 3), "one row: i1 clamped everywhere"),
    ((1, 8, 2, 2), "2x2 (the U-Net's 2x2 -> 4x4); one sample"),
    ((3, 24, 3, 4), "odd height; 216 threads"),
    ((2, 16, 8, 2), "two columns: 2W = 4 row stride"),
    ((3, 24, 10, 12), "the shape of the older test; the tail of q_decode"),
    ((2, 32, 32, 32), "32x32 -> 64x64: 16384 units per sample"),
]
# ghm_bn_backward_hi, (N, K, H, W) of the low-resolution map
HI_BWD_ROWS = [
    ((2, 8, 1, 1), "S = 1, a 1x1 low-resolution map, one channel block"),
    ((3, 24, 10, 12), "the shape of the older test: S = 1 (count / 512 == 0)"),
    ((3, 16, 21, 17), "count 1071: S = 2, chunks 536 + 535 (ragged), odd W (rows 8-byte aligned only), workspace stride max_split"),
    ((2, 512, 32, 32), "count 2048, K = 512: S = 4 where the 2048 / K cap and the count / 512 cap meet"),
]
# ghm_maxpool2_mask_bwd_q, (N, C, H, W) of the FULL-resolution map (even H, W % 4 == 0)
POOL_ROWS = [
    ((1, 8, 2, 4), "one window pair per (sample, block): bpp = 1, 252 (255) dead lanes; one channel block, one sample"),
    ((3, 24, 20, 28), "the shape of the older test: 280 columns -> bpp = 2; windows: 70 items, bpp = 1"),
    ((2, 16, 36, 20), "columns: 360 items, bpp = 2, dead lanes in the last block, bias partials over N bpp = 4 entries"),
    ((2, 16, 72, 40), "windows: 360 items, bpp = 2; columns: 1440 items, bpp = 6"),
    ((2, 64, 128, 128), "net-sized: more than 2^16 units per plane; bpp = 32 / 8"),
]
# ghm_copy_view / ghm_act_fwd / ghm_act_bwd, (N, C, H, W)
VIEW_ROWS = [((2, 6, 16, 12), "HW % 4 == 0: VEC = 4"), ((3, 5, 7, 9), "HW = 63: VEC = 1")]


# ---- the input sets ----
def _rng(shape, salt):
    return np.random.RandomState((sum(s * 131 ** i for i, s in enumerate(shape)) + salt) % (2 ** 31))


def bn_inputs(shape):
    """x with per-channel offsets and spreads; gamma, beta; dout with a non-zero mean and a component along x (so that the two
    per-channel means of the backward are not draws around zero: as in a net, both terms matter)"""
    N, C, H, W = shape
    r = _rng(shape, 1)
    x = (r.randn(*shape) * (0.5 + 2 * r.rand(1, C, 1, 1)) + r.randn(1, C, 1, 1)).astype(np.float32)
    gamma, beta = (r.rand(C) + 0.5).astype(np.float32), r.randn(C).astype(np.float32)
    mean, inv = bn_stats(x)
    xh = (x - mean.reshape(1, C, 1, 1)) * inv.reshape(1, C, 1, 1)
    dout = (r.randn(*shape) + 0.5 + 0.3 * xh).astype(np.float32)
    return dict(x=x, gamma=gamma, beta=beta, mean=mean, inv=inv, dout=dout)


def hi_inputs(shape):
    """the same for a parity-planar tensor [4N, K, H, W] and a gradient in the interleaved layout [N, K, 2H, 2W]"""
    N, K, H, W = shape
    d = bn_inputs((4 * N, K, H, W))
    d['dhi'] = pp_to_hi(d.pop('dout'))
    return d


def pool_inputs(shape):
    """pooled y and dy, and a mask of random nibbles that holds the all-four-tie nibble (15), every single-bit nibble and the
    empty nibble (0), with bit 4 the sign of y"""
    N, C, H, W = shape
    r = _rng(shape, 2)
    ps = (N, C, H // 2, W // 2)
    y, dy = r.randn(*ps).astype(np.float32), r.randn(*ps).astype(np.float32)
    nib = r.randint(0, 16, ps).astype(np.uint8)
    flat = nib.reshape(-1)
    forced = np.array([15, 1, 2, 4, 8, 0], np.uint8)
    flat[r.permutation(flat.size)[:min(forced.size, flat.size)]] = forced[:flat.size]
    mask = (nib | ((y > 0).astype(np.uint8) << 4)).astype(np.uint8)
    return dict(y=y, dy=dy, mask=mask)


def view_inputs(shape):
    r = _rng(shape, 3)
    return dict(x=r.randn(*shape).astype(np.float32), g=r.randn(*shape).astype(np.float32), prev=r.randn(*shape).astype(np.float32))
