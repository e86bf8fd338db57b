"""Float64 definitions, inputs, restated planner, row table and bounds of the small-map convolutions of csrc/conv_small.hip
(sm_gemm_kernel + sm_finish_kernel + sm_q_pack_kernel: maps of 16 x 16 down to 1 x 1, filters up to 5 x 5, stride 1 and 2,
forward product and data gradient, 'bf16' and 'f16'), shared by tests/test_conv_small_ref.py (CPU: validates the reference,
the inputs, the rows' claims through ghm_sm_plan_query and measures the bounds) and tests/test_gpu_conv_small.py (GPU).
numpy only; built on oracle/ops.py and oracle/lp.py.

A geometry is g = (N, C, H, W, K, k, stride, pad): x [N, C, H, W], W [K, C, k, k], y [N, K, Ho, Wo].

Per-element bound of a product:  |got - ref| <= k 2^-24 M.
  ref  the float64 product of the operands rounded to bf16 / fp16 (oracle/lp.py) + bias;
  M    the same product of the absolute values + |bias| (+ |previous value| where it is asked for);
  k    K_BOUND: twice the worst of ``restate32`` over the real-input rows, rounded up -- measured against this reference,
       never from a kernel.  restate32 is the product in fp32 numpy with ONE strictly sequential fp32 accumulator
       (np.cumsum) over (channel, tap row, tap column), then the bias.  The kernels sum in another order (two MFMA chains
       of 16-product blocks per slab, split partials in fixed order, bias first): each is at least as favourable as one
       sequential accumulator, hence the factor 2.  Whatever is measured, k <= n + S + 2 (n products, S splits).  restate32
       is evaluated on every border class and corner (all four parity classes of a stride-2 data gradient are among them)
       and SAMPLE random outputs per row.

BatchNorm in the finishing kernel: the reference is the float64 BatchNorm (biased variance, eps, running mean / inverse std
blended with run_alpha, oracle/ops.py) of the kernel's OWN fp32 conv_out t.  Per element M_bn = (|t| + |mean|) |gamma inv| +
|beta|; K_BN is twice the worst of ``restate32_bn``, the kernel's formula restated in numpy: fp64 sums of the fp32 values, mean
and inv cast to fp32, fmaf(t - mean, gamma inv, beta).  K_MEAN (against mean |t|), K_INV (against inv) and K_RUN (against
|(1 - a) run| + |a stat|) are measured the same way from the restatement.  On the CPU the restatement's t is the rounded
float64 product.
"""
import collections

import numpy as np

from oracle import lp as LP
from oracle import ops as O
from tests.conv_s2_ref import FRONT, REL_L2, VIEWS, view_layout  # noqa: F401  (the named views of tests/canary.py's View / QView)
from tests.elementwise_q_ref import U, rel, worst  # noqa: F401  (re-exported for the two test modules)

MODES = ('bf16', 'f16')
KINDS = ('fwd', 'dgrad')
KIND_CODE = {'fwd': 0, 'dgrad': 1}
SLOPE = 0.25                        # the activation slope of the integer pass: exact in every format
CUS = 256                           # the CU count the host-only queries plan with, and the MI355X's
SAMPLE = 1024                       # random outputs per row on top of the border grid
MAX_LDS = 160 * 1024
BN_EPS, BN_ALPHA = 1e-4, 0.1
BN_SLOPE = float(np.float32(0.2))   # LeakyRectify(0.2) behind the BatchNorm, as the kernel receives it
ZERO_CHANNEL = 3                    # the filter that is all zeros in every BatchNorm row

# ---- the frozen k per (mode, kind): 2 x the worst of restate32 (in the comment), rounded up.  tests/test_conv_small_ref.py
# re-measures and asserts that these are exactly that ----
K_BOUND = {
    ('bf16', 'fwd'): 11, ('bf16', 'dgrad'): 8,           # 5.08  3.74
    ('f16', 'fwd'): 17, ('f16', 'dgrad'): 12,            # 8.04  5.52
    ('f32', 'fwd'): 7,                                   # 3.30  (the conv_out of the one fp32 BatchNorm row: products rounded)
}
# the BatchNorm of the finishing kernel: 2 x the worst of restate32_bn over BN_ROWS, rounded up
K_BN = 7                            # 3.11  y against M_bn
K_MEAN = 2                          # 0.98  the batch mean against mean |t|
K_INV = 2                           # 0.93  the inverse standard deviation against itself
K_RUN = 4                           # 1.76  the running statistics against |(1 - a) run| + |a stat|


def out_hw(g):
    N, C, H, W, K, k, s, pad = g
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def shapes(g):
    N, C, H, W, K, k, s, pad = g
    Ho, Wo = out_hw(g)
    return (N, C, H, W), (K, C, k, k), (N, K, Ho, Wo)


def out_shape(kind, g):
    xs, ws, ys = shapes(g)
    return ys if kind == 'fwd' else xs


def in_shape(kind, g):
    xs, ws, ys = shapes(g)
    return xs if kind == 'fwd' else ys


def n_products(kind, g):
    N, C, H, W, K, k, s, pad = g
    return (C if kind == 'fwd' else K) * k * k


# ---- reference ----
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def ref(kind, g, x, W, b, dy):
    """float64: 'fwd' conv(x, W) + b; 'dgrad' conv^T(dy, W) + b (b per INPUT channel, the epilogue bias of the data-gradient
    entry points).  b None: no bias."""
    N, C, H, Wd, K, k, s, pad = g
    x, W, b, dy = _f64(x), _f64(W), _f64(b), _f64(dy)
    if kind == 'fwd':
        return O.conv2d_fwd(x, W, b if b is not None else np.zeros(K), s, pad)
    dx = O.conv2d_vjp(np.zeros((N, C, H, Wd)), W, dy, s, pad)[0]
    return dx if b is None else dx + b[None, :, None, None]


def ref_mode(mode, kind, g, x, W, b, dy):
    """the float64 answer the mode is held to: the operands rounded first"""
    r = LP.ROUND[mode]
    return ref(kind, g, None if x is None else r(x), r(W), b, None if dy is None else r(dy))


def M(mode, kind, g, x, W, b, dy, prev=None):
    """sum |a| |b| + |bias| + |prev| in float64, the operands rounded first"""
    r = LP.ROUND[mode]
    ab = lambda v: None if v is None else np.abs(_f64(r(v)))       # noqa: E731
    m = ref(kind, g, ab(x), ab(W), None if b is None else np.abs(_f64(b)), ab(dy))
    return m if prev is None else m + np.abs(_f64(prev))


# ---- the product as explicit dot products at chosen outputs ----
def terms(kind, g, A, B, idx):
    """-> (a, b) of shape [len(idx), n]: out[idx[e]] = sum_t a[e, t] b[e, t] (taps on padding, or between the samples of a
    stride-2 gradient, are zero terms); A the operand map (x / dy), B the filter; idx integer [E, 4]"""
    N, C, H, W, K, k, s, pad = g
    A, B, idx = np.asarray(A), np.asarray(B), np.asarray(idx)
    E, ar = len(idx), np.arange(k)
    Bf = B[:, :, ::-1, ::-1]
    if kind == 'fwd':                       # idx (n, ko, i, j); reduction order (c, a, b)
        xp = np.pad(A, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        n, ko, i, j = idx.T
        rows = (s * i)[:, None, None] + ar[None, :, None]
        cols = (s * j)[:, None, None] + ar[None, None, :]
        a = xp[n[:, None, None, None], np.arange(C)[None, :, None, None], rows[:, None], cols[:, None]]
        b = Bf[ko]
        return a.reshape(E, -1), b.reshape(E, -1)
    Ho, Wo = out_hw(g)                      # idx (n, c, h, w); reduction order (ko, a, b); s i + a = h + pad
    Z = np.zeros((N, K, H + pad + k - 1, W + pad + k - 1), A.dtype)
    Z[:, :, k - 1:k - 1 + s * Ho:s, k - 1:k - 1 + s * Wo:s] = A
    n, c, h, w = idx.T
    rows = (h + pad + k - 1)[:, None, None] - ar[None, :, None]
    cols = (w + pad + k - 1)[:, None, None] - ar[None, None, :]
    a = Z[n[:, None, None, None], np.arange(K)[None, :, None, None], rows[:, None], cols[:, None]]
    b = Bf[:, c].transpose(1, 0, 2, 3)
    return a.reshape(E, -1), b.reshape(E, -1)


def hash_g(g):
    return sum(int(s) * 131 ** i for i, s in enumerate(g))


def sample_idx(kind, g, salt=0, count=SAMPLE):
    """output indices for restate32: every combination of {0, 1, last - 1, last} over the four axes (every border class, every
    corner, all four parity classes) and ``count`` random ones"""
    shp = out_shape(kind, g)
    edge = [sorted({0, min(1, s - 1), max(s - 2, 0), s - 1}) for s in shp]
    grid = np.stack(np.meshgrid(*edge, indexing='ij'), -1).reshape(-1, 4)
    r = np.random.RandomState((hash_g(g) + 17 * salt + 5) % (2 ** 31))
    rnd = np.stack([r.randint(0, s, count) for s in shp], -1)
    return np.concatenate([grid, rnd])


def restate32(kind, mode, g, x, W, b, dy, idx):
    """the product in fp32 numpy at the outputs ``idx``: products of bf16 / fp16 operands (exact in fp32), ONE sequential fp32
    accumulator, then the bias"""
    r = LP.ROUND[mode]
    ta, tb = terms(kind, g, r(x if kind == 'fwd' else dy), r(W), idx)
    acc = np.cumsum(ta.astype(np.float32) * tb.astype(np.float32), axis=1, dtype=np.float32)[:, -1]
    if b is not None:
        acc = (acc + np.asarray(b, np.float32)[np.asarray(idx)[:, 1]]).astype(np.float32)
    return acc


def at(a, idx):
    idx = np.asarray(idx)
    return np.asarray(a)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


def element_class(kind, g, index):
    """the border (and, in a stride-2 data gradient, parity) class of an output element, for the failure report"""
    N, C, H, W, K, k, s, pad = g
    shp = out_shape(kind, g)
    def edge(v, n):         # noqa: E306
        return "first" if v == 0 else ("last" if v == n - 1 else "inner")
    text = "%s row, %s column of %d x %d" % (edge(index[2], shp[2]), edge(index[3], shp[3]), shp[2], shp[3])
    if kind == 'dgrad' and s == 2:
        c = 2 * (index[2] % 2) + index[3] % 2
        text += ", parity class %d (%d taps)" % (c, class_taps(g)[c])
    return text


def class_taps(g):
    """taps per output parity class (row parity, column parity) of a stride-2 data gradient"""
    N, C, H, W, K, k, s, pad = g
    per = [sum(1 for a in range(k) if (p + pad - k + 1 + a) % 2 == 0) for p in (0, 1)]
    return tuple(per[c >> 1] * per[c & 1] for c in range(4))


# ---- inputs ----
def _signed(r, hi, shape):
    return (r.randint(1, hi + 1, shape) * (2 * r.randint(0, 2, shape) - 1)).astype(np.float32)


def int_inputs(g, salt=0):
    """x, dy in +-{1, 2, 3}, W in +-{1, 2}, integer biases and previous values: every partial sum in any order stays below 2^24
    and every operand is exact in bf16 and fp16 -- both modes must return the float64 answer bit for bit"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt) % (2 ** 31))
    d = dict(x=_signed(r, 3, xs), W=_signed(r, 2, ws), dy=_signed(r, 3, ys), b=_signed(r, 4, ws[0]), bc=_signed(r, 4, ws[1]))
    d['prev'] = {k: _signed(r, 7, out_shape(k, g)) for k in KINDS}
    return d


def real_inputs(g, salt=0):
    """randn with per-(sample, channel) scales exp(randn), as tests/conv_s2_ref.py draws them"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt + 1000) % (2 ** 31))
    d = dict(x=(r.randn(*xs) * np.exp(r.randn(xs[0], xs[1], 1, 1))).astype(np.float32),
             W=(r.randn(*ws) / np.sqrt(float(ws[1] * ws[2] * ws[3]))).astype(np.float32),
             dy=(r.randn(*ys) * np.exp(r.randn(ys[0], ys[1], 1, 1))).astype(np.float32),
             b=r.randn(ws[0]).astype(np.float32), bc=r.randn(ws[1]).astype(np.float32))
    d['prev'] = {k: r.randn(*out_shape(k, g)).astype(np.float32) for k in KINDS}
    return d


def bias_of(kind, d):
    return d['b'] if kind == 'fwd' else d['bc']


def int_magnitude(kind, g):
    """an upper bound of sum |a| |b| + |bias| + |prev| of the integer inputs, from their ranges"""
    return 3 * 2 * n_products(kind, g) + 4 + 7


# ---- BatchNorm ----
def bn_inputs(g, salt=0):
    """real inputs of a BatchNorm row: the filter of channel ZERO_CHANNEL is all zeros (its conv_out is its bias everywhere: zero
    variance, the var < 0 clamp's neighbourhood)"""
    d = real_inputs(g, salt + 7)
    K = g[4]
    r = np.random.RandomState((hash_g(g) + salt + 2000) % (2 ** 31))
    d['W'][ZERO_CHANNEL] = 0
    d['gamma'], d['beta'] = (1 + 0.2 * r.randn(K)).astype(np.float32), (0.3 * r.randn(K)).astype(np.float32)
    d['rm'], d['ri'] = r.randn(K).astype(np.float32), (1 + 0.1 * r.rand(K)).astype(np.float32)
    return d


def _ch(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


def act64(v, act, slope=SLOPE):
    if act == 'relu':
        return np.where(v > 0, v, 0.0)
    return v if act == 'linear' else np.where(v > 0, v, slope * v)


def bn_ref(t, d, act='lrelu', slope=SLOPE, eps=BN_EPS, alpha=BN_ALPHA):
    """float64 BatchNorm of the fp32 tensor t -> dict(y, mean, inv, rm, ri, M, M_mean, M_rm, M_ri)"""
    t = np.asarray(t, np.float64)
    eps64, a = float(np.float32(eps)), float(np.float32(alpha))
    mean, var = t.mean(axis=(0, 2, 3)), t.var(axis=(0, 2, 3))
    inv = 1.0 / np.sqrt(var + eps64)
    g64, b64 = np.asarray(d['gamma'], np.float64), np.asarray(d['beta'], np.float64)
    y = (t - _ch(mean)) * _ch(g64 * inv) + _ch(b64)
    rm, ri = np.asarray(d['rm'], np.float64), np.asarray(d['ri'], np.float64)
    return dict(y=act64(y, act, slope), mean=mean, inv=inv, rm=(1 - a) * rm + a * mean, ri=(1 - a) * ri + a * inv,
                M=(np.abs(t) + np.abs(_ch(mean))) * np.abs(_ch(g64 * inv)) + np.abs(_ch(b64)),
                M_mean=np.abs(t).mean(axis=(0, 2, 3)), M_rm=np.abs((1 - a) * rm) + np.abs(a * mean),
                M_ri=np.abs((1 - a) * ri) + np.abs(a * inv))


def _fl(v):
    return np.asarray(v, np.float64).astype(np.float32)


def restate32_bn(t, d, act='lrelu', slope=SLOPE, eps=BN_EPS, alpha=BN_ALPHA):
    """sm_finish_kernel's BatchNorm in numpy: fp64 sums of the fp32 values, var = E[t^2] - mean^2 clamped at 0, mean and inv
    cast to fp32, y = fmaf(t - mean, gamma inv, beta) (the product of two fp32 values is exact in float64), the running
    statistics (1 - a) run + a stat in fp32"""
    t = np.asarray(t, np.float32)
    t64 = t.astype(np.float64)
    n = t64.size // t64.shape[1]
    mu = t64.sum(axis=(0, 2, 3)) / n
    var = np.maximum((t64 * t64).sum(axis=(0, 2, 3)) / n - mu * mu, 0.0)
    mf, iv = _fl(mu), _fl(1.0 / np.sqrt(var + float(np.float32(eps))))
    sc = (np.asarray(d['gamma'], np.float32) * iv).astype(np.float32)
    diff = (t - mf.reshape(1, -1, 1, 1)).astype(np.float32)
    y = _fl(diff.astype(np.float64) * _ch(sc) + _ch(d['beta']))
    y = np.where(y > 0, y, (np.float32(0 if act == 'relu' else (1 if act == 'linear' else slope)) * y).astype(np.float32))
    a = np.float32(alpha)
    one = np.float32(1) - a
    rm = ((one * np.asarray(d['rm'], np.float32)).astype(np.float32) + (a * mf).astype(np.float32)).astype(np.float32)
    ri = ((one * np.asarray(d['ri'], np.float32)).astype(np.float32) + (a * iv).astype(np.float32)).astype(np.float32)
    return dict(y=y.astype(np.float32), mean=mf, inv=iv, rm=rm, ri=ri)


# ---- csrc/conv_small.hip's planner restated ----
def _cd(a, b):
    return (a + b - 1) // b


def _pick(v, classes):
    for c in classes:
        if v <= c:
            return c
    return -1


def ring(ntaps, nq):
    """SmRing<NTAPS, NQ>: (units per slot, DMA instructions per wave and slab, deepest ring)"""
    wi = (ntaps + 3) // 4
    return 4 * wi * 64 + nq * 256, wi + nq, min(8, 60 // (wi + nq) + 2)


def sm_plan(g, kind, env, cus=CUS):
    """sm_plan(d, kind, cus) under the tuning switches ``env`` -> dict or None (not served)"""
    N, C, H, W, K, k, s, pad = g
    if 'GHM_NO_SM' in env or 'GHM_NO_LP' in env or k > 5 or s not in (1, 2):
        return None
    Ho, Wo = out_hw(g)
    if kind == 'fwd':
        CH, Hin, Win, h, w, R, st, ncls, OH, OW = C, H, W, Ho, Wo, K, s, 1, Ho, Wo
    elif s == 1:
        CH, Hin, Win, h, w, R, st, ncls, OH, OW = K, Ho, Wo, H, W, C, 1, 1, H, W
    else:
        if H % 2 or W % 2:
            return None
        CH, Hin, Win, h, w, R, st, ncls, OH, OW = K, Ho, Wo, H // 2, W // 2, C, 1, 4, H, W
    if CH % 16 or CH < 16 or R % 8 or R < 8:
        return None
    HW = h * w
    if HW > 256 or w > 16 or not ((HW >= 128 and HW % 128 == 0 and 128 % w == 0) or (HW < 128 and 128 % HW == 0)):
        return None
    Mcls, Mtot = N * HW, N * OH * OW
    maxm = int(env.get('GHM_SM_MAXM', 1024 if ncls == 4 else 512))
    if Mcls > maxm or Mtot > 8192:
        return None
    nimg, rows = (1, 128 // w) if HW >= 128 else (min(128 // HW, N), h)
    if ncls == 1:
        cnts, span_y, span_x = [k * k], k - 1, k - 1
    else:
        cnts, ys, xs = [], [], []
        for c in range(4):
            n = 0
            for ta in range(k):
                ey = (c >> 1) + pad - k + 1 + ta
                if ey & 1:
                    continue
                for tb in range(k):
                    ex = (c & 1) + pad - k + 1 + tb
                    if ex & 1:
                        continue
                    ys.append(int(ey / 2))           # (C division: towards zero)
                    xs.append(int(ex / 2))
                    n += 1
            cnts.append(n)
        if sum(cnts) > 36:
            return None
        span_y, span_x = max(ys) - min(ys), max(xs) - min(xs)
    LH, LW = (rows - 1) * st + span_y + 1, (w - 1) * st + span_x + 1
    ntaps, nq = _pick(max(cnts), (4, 9, 25)), _pick(_cd(2 * nimg * LH * LW, 256), (1, 2, 5))
    if ntaps < 0 or nq < 0:
        return None
    ftiles, pgroups, nslabs = _cd(R, 32), _cd(Mcls, 128), CH // 16
    splits = min(8, _cd(cus, ftiles * pgroups * ncls))
    if 'GHM_SM_SPLITS' in env:
        splits = int(env['GHM_SM_SPLITS'])
    splits = max(1, min(splits, nslabs))
    sps = _cd(nslabs, splits)
    splits = _cd(nslabs, sps)
    slot, G, maxpfs = ring(ntaps, nq)
    budget = min(int(env.get('GHM_SM_LDS_KB', 32)) * 1024, MAX_LDS)
    pfs = max(min(budget // (slot * 16), maxpfs, sps + 1), 3)
    return dict(ncls=ncls, cls=tuple(cnts), ntaps=ntaps, nq=nq, nimg=nimg, rows=rows, splits=splits, sps=sps, pfs=pfs,
                lds=pfs * slot * 16, finish=256 if Mtot <= 256 else (1024 if Mtot <= 1024 else 0), nslabs=nslabs,
                last=nslabs - (splits - 1) * sps, pixels=Mtot, grid=(ftiles, pgroups, ncls * splits))


CLAIM = ('ntaps', 'nq', 'cls', 'nimg', 'rows', 'splits', 'sps', 'pfs')


def claim(p):
    return tuple(p[f] for f in CLAIM)


# ---- the row table ----
Row = collections.namedtuple('Row', 'mode kind g view env reaches why')
SPLIT1 = {'GHM_SM_SPLITS': '1'}
RING_KB = (32, 64, 96, 128, 160)
RING_SHAPES = [('fwd', (3, 112, 4, 4, 16, 3, 1, 1)), ('dgrad', (3, 16, 4, 4, 112, 3, 2, 1)), ('fwd', (2, 96, 4, 4, 8, 5, 1, 2)),
               ('fwd', (2, 160, 16, 16, 8, 3, 1, 1))]

# (kind(s), g, env, {kind: (ntaps, nq, taps per class, images, rows, splits, slabs per split, ring slots)}, why)
_ROWS = [
    (('fwd',), (2, 16, 32, 32, 16, 2, 2, 0), {}, {'fwd': (4, 5, (4,), 1, 8, 1, 1, 3)},
     "variant (4, 5): a 2x2 stride-2 forward from 32 x 32 stages a 15 x 31 window"),
    (('fwd', 'dgrad'), (2, 16, 32, 32, 16, 3, 2, 1), {},
     {'fwd': (9, 5, (9,), 1, 8, 1, 1, 3), 'dgrad': (4, 2, (1, 2, 2, 4), 1, 8, 1, 1, 3)},
     "(9, 5); parity classes 1 / 2 / 2 / 4 on 16 x 16 class maps, 2048 outputs per channel (8 finishing blocks)"),
    (('fwd', 'dgrad'), (3, 16, 8, 8, 16, 4, 2, 1), {},
     {'fwd': (25, 5, (16,), 3, 4, 1, 1, 3), 'dgrad': (4, 1, (4, 4, 4, 4), 3, 4, 1, 1, 3)},
     "4x4 filter: 16 taps in the 25 class (9 zero weight rows); classes 4 / 4 / 4 / 4; three images in one block"),
    (('fwd', 'dgrad'), (2, 16, 32, 32, 16, 4, 2, 1), {},
     {'fwd': (25, 5, (16,), 1, 8, 1, 1, 3), 'dgrad': (4, 2, (4, 4, 4, 4), 1, 8, 1, 1, 3)}, "the same from 32 x 32: row ranges of one image"),
    (('dgrad',), (3, 16, 8, 8, 16, 5, 2, 2), {}, {'dgrad': (9, 1, (9, 6, 6, 4), 3, 4, 1, 1, 3)}, "5x5 stride 2: classes 9 / 6 / 6 / 4, (9, 1)"),
    (('dgrad',), (2, 16, 16, 16, 16, 5, 2, 2), {}, {'dgrad': (9, 2, (9, 6, 6, 4), 2, 8, 1, 1, 3)}, "the same on 8 x 8 classes: (9, 2)"),
    (('dgrad',), (3, 24, 4, 4, 16, 2, 2, 0), {}, {'dgrad': (4, 1, (1, 1, 1, 1), 3, 2, 1, 1, 3)}, "2x2 stride 2: classes 1 / 1 / 1 / 1; 24 rows"),
    (('fwd', 'dgrad'), (2, 16, 1, 1, 16, 1, 1, 0), {}, {'fwd': (4, 1, (1,), 2, 1, 1, 1, 3), 'dgrad': (4, 1, (1,), 2, 1, 1, 1, 3)},
     "1x1 filter on a 1 x 1 map: two pixels in all"),
    (('fwd',), (5, 16, 4, 4, 24, 1, 1, 0), {}, {'fwd': (4, 1, (1,), 5, 4, 1, 1, 3)}, "1x1 filter, 24 filters, five images"),
    (('fwd',), (3, 16, 2, 2, 8, 2, 1, 0), {}, {'fwd': (4, 1, (4,), 3, 1, 1, 1, 3)}, "3 pixels, 8 filters (a quarter row tile)"),
    (('fwd', 'dgrad'), (5, 16, 2, 2, 16, 3, 1, 1), {}, {'fwd': (9, 1, (9,), 5, 2, 1, 1, 3), 'dgrad': (9, 1, (9,), 5, 2, 1, 1, 3)},
     "20 pixels; a window that is mostly padding"),
    (('fwd', 'dgrad'), (2, 16, 16, 8, 16, 3, 1, 1), {}, {'fwd': (9, 2, (9,), 1, 16, 1, 1, 3), 'dgrad': (9, 2, (9,), 1, 16, 1, 1, 3)},
     "non-square 16 x 8: one image per block"),
    (('fwd', 'dgrad'), (3, 16, 4, 8, 16, 3, 1, 1), {}, {'fwd': (9, 2, (9,), 3, 4, 1, 1, 3), 'dgrad': (9, 2, (9,), 3, 4, 1, 1, 3)},
     "non-square 4 x 8: three of four images"),
    (('fwd', 'dgrad'), (3, 16, 16, 4, 16, 5, 1, 2), {}, {'fwd': (25, 5, (25,), 2, 16, 1, 1, 3), 'dgrad': (25, 5, (25,), 2, 16, 1, 1, 3)},
     "non-square 16 x 4, 5x5: (25, 5); the second pixel group holds one image of two"),
    (('fwd',), (3, 32, 8, 8, 40, 3, 1, 1), {}, {'fwd': (9, 2, (9,), 2, 8, 2, 1, 3)}, "40 filters (32 + 8); N = 3 with two images per block"),
    (('dgrad',), (3, 40, 8, 8, 32, 3, 1, 1), {}, {'dgrad': (9, 2, (9,), 2, 8, 2, 1, 3)}, "40 input channels: the ragged row tile of a data gradient"),
    (('fwd',), (2, 48, 16, 16, 24, 3, 1, 1), {}, {'fwd': (9, 2, (9,), 1, 8, 3, 1, 3)}, "24 filters; 16 x 16 in two row ranges per image"),
    (('fwd',), (1, 16, 16, 16, 8, 5, 1, 2), {}, {'fwd': (25, 2, (25,), 1, 8, 1, 1, 3)}, "8 filters, 5x5: (25, 2)"),
    (('fwd', 'dgrad'), (5, 32, 4, 4, 16, 3, 1, 1), {}, {'fwd': (9, 2, (9,), 5, 4, 2, 1, 3), 'dgrad': (9, 2, (9,), 5, 4, 1, 1, 3)},
     "5 images in an 8-image group"),
    (('fwd', 'dgrad'), (9, 16, 4, 4, 16, 3, 1, 1), {}, {'fwd': (9, 5, (9,), 8, 4, 1, 1, 3), 'dgrad': (9, 5, (9,), 8, 4, 1, 1, 3)},
     "nine images in groups of eight: the second block stages one image and seven empty windows"),
    (('fwd',), (2, 16, 4, 4, 160, 3, 1, 1), {}, {'fwd': (9, 1, (9,), 2, 4, 1, 1, 3)}, "160 filters: five row tiles, pack rows padded to 256"),
    (('dgrad',), (2, 160, 4, 4, 16, 3, 1, 1), {}, {'dgrad': (9, 1, (9,), 2, 4, 1, 1, 3)}, "160 input channels: the same in the transposed pack"),
    (('fwd',), (2, 256, 4, 4, 16, 3, 1, 1), {}, {'fwd': (9, 1, (9,), 2, 4, 8, 2, 3)}, "the plan's own eight splits of two slabs each, as in the nets"),
    (('fwd',), (3, 144, 4, 4, 16, 3, 1, 1), {'GHM_SM_SPLITS': '16'}, {'fwd': (9, 1, (9,), 3, 4, 9, 1, 3)},
     "9 splits: the second round of the finishing kernel's loop holds one partial"),
    (('fwd',), (2, 160, 16, 16, 8, 3, 1, 1), {'GHM_SM_SPLITS': '16'}, {'fwd': (9, 2, (9,), 1, 8, 10, 1, 3)}, "10 splits, 512 pixels"),
    (('dgrad',), (4, 32, 4, 4, 80, 3, 2, 1), {'GHM_SM_SPLITS': '3'}, {'dgrad': (4, 1, (1, 2, 2, 4), 4, 2, 3, 2, 3)},
     "5 slabs in splits of 2 + 2 + 1: a ragged last split"),
]
# ring depths: one split, 6 .. 10 slabs per block at GHM_SM_LDS_KB = 32, 64, 96, 128, 160 -> the ring slots below
_RING_PFS = [(3, 4, 6, 8, 8), (4, 8, 8, 8, 8), (3, 3, 3, 4, 5), (3, 3, 4, 6, 8)]
_RING_CLAIM = [(9, 1, (9,), 3, 4, 1, 7), (4, 1, (1, 2, 2, 4), 3, 2, 1, 7), (25, 1, (25,), 2, 4, 1, 6), (9, 2, (9,), 1, 8, 1, 10)]
for (_kind, _g), _c, _pfs in zip(RING_SHAPES, _RING_CLAIM, _RING_PFS):
    for _kb, _p in zip(RING_KB, _pfs):
        _ROWS.append(((_kind,), _g, dict(SPLIT1, GHM_SM_LDS_KB=str(_kb)), {_kind: _c + (_p,)},
                      "%d slabs in one block round a ring of %d slots" % (_c[6], _p)))
# 32 slabs in one block, as the nets' 512-channel layers walk them, at EVERY ring depth 3 .. 8 (depth 7 included: 56 KB of
# 8 KB slots): at least 2 pfs + 1 slabs, so every slot is reused twice or more
DEEP = (2, 16, 4, 4, 512, 3, 2, 1)
DEEP_KB = ((24, 3), (32, 4), (40, 5), (48, 6), (56, 7), (64, 8))
for _kb, _p in DEEP_KB:
    _ROWS.append((('dgrad',), DEEP, dict(SPLIT1, GHM_SM_LDS_KB=str(_kb)), {'dgrad': (4, 1, (1, 2, 2, 4), 2, 2, 1, 32, _p)},
                  "32 slabs in one block round a ring of %d slots" % _p))


def _rows():
    out, v = [], 0
    for kinds, g, env, reaches, why in _ROWS:
        for kind in kinds:
            for m in MODES:
                out.append(Row(m, kind, g, VIEWS[v % 3], env, reaches[kind], why))
            v += 1
    return out


ROWS = _rows()


def row_id(r):
    return "%s-%s-%s-%s%s" % (r.mode, r.kind, "x".join(str(v) for v in r.g), r.view,
                              "".join("-%s=%s" % (k.replace('GHM_SM_', ''), v) for k, v in sorted(r.env.items())))


# BatchNorm rows: (path, g, env, (finishing form, pixels per channel, splits), why); path 'sm' (sm_conv), 'splitk'
# (lp_conv_kernel in split-K form -> lp_fwd_splitk_bn) or 'f32' (ghm_conv2d_bn_fwd: igemm partials + the same finishing kernel)
BnRow = collections.namedtuple('BnRow', 'path g env reaches why')
BN_ROWS = [
    BnRow('sm', (2, 16, 1, 1, 16, 1, 1, 0), {}, (256, 2, 1), "2 pixels per channel: one lane of a half-wave holds a value"),
    BnRow('sm', (5, 16, 2, 2, 16, 3, 1, 1), {}, (256, 20, 1), "20 pixels"),
    BnRow('sm', (3, 32, 4, 4, 16, 3, 1, 1), {}, (256, 48, 2), "48 pixels, two splits"),
    BnRow('sm', (3, 16, 8, 8, 16, 3, 1, 1), {}, (256, 192, 1), "192 pixels: the last two of a thread's eight are masked"),
    BnRow('sm', (4, 16, 8, 8, 16, 3, 1, 1), {}, (256, 256, 1), "256 pixels: the <256> form full"),
    BnRow('sm', (5, 32, 8, 8, 16, 3, 1, 1), {}, (1024, 320, 2), "320 pixels in the <1024> form: five of a thread's eight masked, in every wave"),
    BnRow('sm', (3, 32, 16, 16, 16, 3, 1, 1), {'GHM_SM_MAXM': '1024'}, (1024, 768, 2), "768 pixels"),
    BnRow('sm', (4, 16, 16, 16, 16, 3, 1, 1), {'GHM_SM_MAXM': '1024'}, (1024, 1024, 1), "1024 pixels: the <1024> form full"),
    BnRow('splitk', (3, 160, 16, 16, 32, 3, 1, 1), {'GHM_LP_SPLITS': '10'}, (1024, 768, 10),
     "lp_conv_kernel's split-K partials (lp_fwd_splitk_bn): ten of them, the finishing loop's second round, 768 pixels"),
    BnRow('f32', (3, 32, 8, 8, 16, 3, 1, 1), {}, (256, 192, 0), "ghm_conv2d_bn_fwd: the fp32 gather kernel's partials, the same finishing kernel"),
]


def bn_row_id(r):
    return "%s-%s%s" % (r.path, "x".join(str(v) for v in r.g), "".join("-%s=%s" % (k.replace('GHM_', ''), v) for k, v in sorted(r.env.items())))


def lp_splits(g, env, cus=CUS):
    """the split count of lp_plan (csrc/conv_lp.hip) for a stride-1 'same' 16 x 16 forward (the 'splitk' BatchNorm rows)"""
    N, C, H, W, K, k, s, pad = g
    assert s == 1 and W % 32 and W % 16 == 0 and H % 8 == 0 and K >= 32 and C % 16 == 0 and k in (3, 5)
    grid, nslabs, splits = _cd(K, 64) * (W // 16) * (H // 8) * N, C // 16, 1
    if grid < cus:
        splits = min(_cd(2 * cus, grid), max(nslabs // 2, 1))
    if 'GHM_LP_SPLITS' in env:
        f = int(env['GHM_LP_SPLITS'])
        splits = (f if f > 0 else 1) if f < nslabs else nslabs
    return _cd(nslabs, _cd(nslabs, splits))
