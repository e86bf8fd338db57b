"""Float64 definitions, inputs, row table and bounds of the 3x3 stride-2 pad-1 convolutions (H = 2 Ho, W = 2 Wo) in the five
arithmetic modes, shared by tests/test_conv_s2_ref.py (CPU: validates the reference, the inputs, the rows' claims and measures
the bound) and tests/test_gpu_conv_s2.py (GPU).  numpy only; built on oracle/ops.py and oracle/lp.py.

Geometry: y[n, k, i, j] = b[k] + sum_{c, a, b} xpad[n, c, 2 i + a, 2 j + b] Wc[k, c, a, b], Wc the flipped filter (Lasagne's
true convolution).  Output row i reads input rows 2 i - 1 .. 2 i + 1: the top and left padding is read, the bottom and right
padding never is.  In the data gradient an even row receives one tap row and an odd row two.

Per-element bound of every product:  |got - ref| <= k 2^-24 M.
  ref  the float64 product of the operands the mode multiplies: the fp32 operands ('f32', 'bf16x3'), the operands rounded to
       bf16 / fp16 ('bf16', 'f16'), the three kept piece products of the two-piece operands ('bf16x2');
  M    the same product of the absolute values, + |bias| (+ |previous value| where a finish adds it among its partials);
  k    K_BOUND below: twice the worst of ``restate32`` over the real-input rows, rounded up -- measured against this
       reference, never from a kernel.  restate32 is the product in fp32 numpy with rounded products and ONE strictly
       sequential fp32 accumulator (np.cumsum); the split modes run their six / three kept piece products through the same
       accumulator.  The kernels sum in other orders (MFMA blocks of 2 or 16 products, split-K partials, the split kernels'
       leading and correction accumulators): each is at least as favourable as one sequential accumulator, hence the factor 2.
       Whatever is measured, k <= n + S + 2 (n products per output, S splits): the forward error bound of an fp32 sum in any
       order.  restate32 is evaluated on a sample of outputs per row (every border class and corner, and SAMPLE random ones).
"""
import collections

import numpy as np

from oracle import lp as LP
from oracle import ops as O
from tests.elementwise_q_ref import U, pieces, rel, worst  # noqa: F401  (re-exported for the two test modules)

MODES = ('f32', 'bf16', 'f16', 'bf16x3', 'bf16x2')
KINDS = ('fwd', 'dgrad', 'wgrad')
KIND_CODE = {'fwd': 0, 'dgrad': 1, 'wgrad': 2}
SLOPE = 0.25                        # the activation slope of the integer pass: exact in every format
REL_L2 = {'f32': 1e-5, 'bf16': 2e-5, 'f16': 2e-5, 'bf16x3': 2e-6, 'bf16x2': 2e-6}      # the bounds of the older tests
CUS = 256                           # the CU count the host-only queries plan with, and the MI355X's
SAMPLE = 4096                       # per row; the GPU module compares 10^4 .. 10^5 elements per call, so the maximum needs a sample of that order

# ---- the frozen k per (mode, kind): 2 x the worst of restate32 (in the comment), rounded up.  tests/test_conv_s2_ref.py
# re-measures and asserts that these are exactly that ----
K_BOUND = {
    ('f32', 'fwd'): 13, ('f32', 'dgrad'): 10, ('f32', 'wgrad'): 11,             # 6.32  4.85  5.35
    ('bf16', 'fwd'): 9, ('bf16', 'dgrad'): 7, ('bf16', 'wgrad'): 10,            # 4.26  3.06  4.57
    ('f16', 'fwd'): 12, ('f16', 'dgrad'): 14, ('f16', 'wgrad'): 8,              # 5.52  6.71  3.93
    ('bf16x3', 'fwd'): 44, ('bf16x3', 'dgrad'): 21, ('bf16x3', 'wgrad'): 22,    # 21.54  10.37  10.89
    ('bf16x2', 'fwd'): 39, ('bf16x2', 'dgrad'): 20, ('bf16x2', 'wgrad'): 22,    # 19.31  9.78  10.60
}
# (the split modes' restatement adds 6 n / 3 n terms to ONE accumulator, the corrections onto the finished leading sum: its
# worst is 3 - 4 times the plain modes'.  The scaled inputs (exp(randn) per sample and channel) have heavier tails than plain
# randn data, for which a trial gave 3.3 - 4.1: a few dominant channels carry the sum early and every later addition rounds
# at their magnitude.)


def shapes(g):
    N, C, H, W, K = g
    return (N, C, H, W), (K, C, 3, 3), (N, K, H // 2, W // 2)


def out_shape(kind, g):
    xs, ws, ys = shapes(g)
    return {'fwd': ys, 'dgrad': xs, 'wgrad': ws}[kind]


def n_products(kind, g):
    N, C, H, W, K = g
    return {'fwd': 9 * C, 'dgrad': 9 * K, 'wgrad': N * (H // 2) * (W // 2)}[kind]


# ---- reference ----
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def ref(kind, x, W, b, dy):
    """float64: 'fwd' conv(x, W) + b; 'dgrad' conv^T(dy, W) + b (b per INPUT channel, the epilogue bias of the data-gradient
    entry points; x only gives the shape); 'wgrad' the gradient of W.  b None: no bias."""
    x, W, b, dy = _f64(x), _f64(W), _f64(b), _f64(dy)
    if kind == 'fwd':
        return O.conv2d_fwd(x, W, b if b is not None else np.zeros(W.shape[0]), 2, 1)
    if kind == 'dgrad':
        dx = O.conv2d_vjp(np.zeros((dy.shape[0], W.shape[1], 2 * dy.shape[2], 2 * dy.shape[3])), W, dy, 2, 1)[0]
        return dx if b is None else dx + b[None, :, None, None]
    assert kind == 'wgrad'
    return O.conv2d_vjp(x, np.zeros((dy.shape[1], x.shape[1], 3, 3)), dy, 2, 1)[1]


def operands(kind, x, W, dy):
    """the two operands the product multiplies (A, B), and how to put them back into ref's arguments"""
    if kind == 'fwd':
        return x, W, lambda a, b_: dict(x=a, W=b_, dy=None)
    if kind == 'dgrad':
        return dy, W, lambda a, b_: dict(x=None, W=b_, dy=a)
    return x, dy, lambda a, b_: dict(x=a, W=None, dy=b_)


def piece_pairs(mode, A, B):
    """the (A piece, B piece) pairs whose products the mode sums, leading product first"""
    A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
    if mode == 'f32':
        return [(A, B)]
    if mode in ('bf16', 'f16'):
        r = LP.ROUND[mode]
        return [(r(A), r(B))]
    pa, pb = pieces(A, mode), pieces(B, mode)
    terms = LP.split_product_terms() if mode == 'bf16x3' else LP.split2_product_terms()
    return [(pa[i], pb[j]) for i, j in sorted(terms, key=lambda t: (t[0] + t[1], t))]


def ref_mode(mode, kind, x, W, b, dy):
    """the float64 answer the mode is held to"""
    A, B, back = operands(kind, x, W, dy)
    if mode in ('f32', 'bf16x3'):
        return ref(kind, b=b, **back(A, B))
    out = 0.0
    for a, b_ in piece_pairs(mode, A, B):       # one pair for bf16 / f16, the three kept products for bf16x2
        out = out + ref(kind, b=None, **back(a, b_))
    return out if b is None or kind == 'wgrad' else out + _f64(b)[None, :, None, None]


def M(mode, kind, x, W, b, dy, prev=None):
    """sum |a| |b| + |bias| + |prev| in float64 (the operands rounded first in 'bf16' / 'f16')"""
    A, B, back = operands(kind, x, W, dy)
    if mode in ('bf16', 'f16'):
        A, B = LP.ROUND[mode](A), LP.ROUND[mode](B)
    m = ref(kind, b=None if b is None else np.abs(_f64(b)), **back(np.abs(_f64(A)), np.abs(_f64(B))))
    return m if prev is None else m + np.abs(_f64(prev))


# ---- the product as explicit dot products at chosen outputs ----
def terms(kind, A, B, idx):
    """-> (a, b) of shape [len(idx), n]: out[idx[e]] = sum_t a[e, t] b[e, t] (taps that fall on padding are zero terms);
    idx: integer array [E, 4] of output indices"""
    A, B, idx = np.asarray(A), np.asarray(B), np.asarray(idx)
    E = len(idx)
    ar = np.arange(3)
    if kind == 'fwd':                       # A = x, B = W; idx (n, k, i, j); reduction order (c, a, b)
        xp = np.pad(A, ((0, 0), (0, 0), (1, 1), (1, 1)))
        n, k, i, j = idx.T
        rows = (2 * i)[:, None, None] + ar[None, :, None]
        cols = (2 * j)[:, None, None] + ar[None, None, :]
        a = xp[n[:, None, None, None], np.arange(A.shape[1])[None, :, None, None], rows[:, None], cols[:, None]]
        b = B[:, :, ::-1, ::-1][k]
        return a.reshape(E, -1), b.reshape(E, -1)
    if kind == 'dgrad':                     # A = dy, B = W; idx (n, c, h, w); reduction order (k, a, b)
        N, K, Ho, Wo = A.shape
        dyp = np.zeros((N, K, 2 * Ho + 2, 2 * Wo + 2), A.dtype)
        dyp[:, :, 1:1 + 2 * Ho:2, 1:1 + 2 * Wo:2] = A          # dyp[r + 1] = dy[r / 2] at even r, 0 elsewhere
        n, c, h, w = idx.T
        rows = (h + 2)[:, None, None] - ar[None, :, None]        # r = h + 1 - a
        cols = (w + 2)[:, None, None] - ar[None, None, :]
        a = dyp[n[:, None, None, None], np.arange(K)[None, :, None, None], rows[:, None], cols[:, None]]
        b = B[:, :, ::-1, ::-1][:, c].transpose(1, 0, 2, 3)
        return a.reshape(E, -1), b.reshape(E, -1)
    assert kind == 'wgrad'                  # A = x, B = dy; idx (k, c, a', b') of dW; reduction order (n, i, j)
    xp = np.pad(A, ((0, 0), (0, 0), (1, 1), (1, 1)))
    N, K, Ho, Wo = B.shape
    k, c, a_, b_ = idx.T
    rows = 2 * np.arange(Ho)[None, :, None] + (2 - a_)[:, None, None]
    cols = 2 * np.arange(Wo)[None, None, :] + (2 - b_)[:, None, None]
    a = xp[np.arange(N)[None, :, None, None], c[:, None, None, None], rows[:, None], cols[:, None]]
    b = B[:, k].transpose(1, 0, 2, 3)
    return a.reshape(E, -1), b.reshape(E, -1)


def sample_idx(kind, g, salt=0, count=SAMPLE):
    """output indices for restate32: every combination of {0, 1, last - 1, last} over the four axes (every border parity
    class and corner) and ``count`` random ones"""
    shp = out_shape(kind, g)
    edge = [sorted({0, min(1, s - 1), max(s - 2, 0), s - 1}) for s in shp]
    grid = np.stack(np.meshgrid(*edge, indexing='ij'), -1).reshape(-1, 4)
    r = np.random.RandomState((hash_g(g) + 17 * salt + 5) % (2 ** 31))
    rnd = np.stack([r.randint(0, s, count) for s in shp], -1)
    return np.concatenate([grid, rnd])


def restate32(kind, mode, x, W, b, dy, idx):
    """the product in fp32 numpy at the outputs ``idx``: every kept piece product rounded to fp32 (piece products of bf16 /
    fp16 operands are exact there), ONE sequential fp32 accumulator over all of them, then the bias"""
    A, B, _ = operands(kind, x, W, dy)
    prods = []
    for a, b_ in piece_pairs(mode, A, B):
        ta, tb = terms(kind, a, b_, idx)
        prods.append(ta.astype(np.float32) * tb.astype(np.float32))
    acc = np.cumsum(np.concatenate(prods, axis=1), axis=1, dtype=np.float32)[:, -1]
    if b is not None and kind != 'wgrad':
        acc = (acc + np.asarray(b, np.float32)[np.asarray(idx)[:, 1]]).astype(np.float32)
    return acc


def at(a, idx):
    idx = np.asarray(idx)
    return np.asarray(a)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


# ---- inputs ----
def hash_g(g):
    return sum(int(s) * 131 ** i for i, s in enumerate(g))


def _signed(r, hi, shape):
    return (r.randint(1, hi + 1, shape) * (2 * r.randint(0, 2, shape) - 1)).astype(np.float32)


def int_inputs(g, salt=0):
    """x, dy in +-{1, 2, 3}, W in +-{1, 2}, integer biases and previous values, an activation operand with both signs and exact
    zeros: every partial sum in any order stays below 2^24, every operand is exact in bf16 and fp16 and its second and third
    split pieces are zero -- all five modes must return the float64 answer bit for bit"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt) % (2 ** 31))
    d = dict(x=_signed(r, 3, xs), W=_signed(r, 2, ws), dy=_signed(r, 3, ys), b=_signed(r, 4, ws[0]), bc=_signed(r, 4, ws[1]))
    d['prev'] = {k: _signed(r, 7, out_shape(k, g)) for k in KINDS}
    d['yact'] = r.randint(-2, 3, xs).astype(np.float32)
    return d


def real_inputs(g, salt=0):
    """randn with per-(sample, channel) scales exp(randn), as tests/test_gpu_split.py draws them: every split piece non-zero"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt + 1000) % (2 ** 31))
    d = dict(x=(r.randn(*xs) * np.exp(r.randn(xs[0], xs[1], 1, 1))).astype(np.float32),
             W=(r.randn(*ws) / np.sqrt(9.0 * ws[1])).astype(np.float32),
             dy=(r.randn(*ys) * np.exp(r.randn(ys[0], ys[1], 1, 1))).astype(np.float32),
             b=r.randn(ws[0]).astype(np.float32), bc=r.randn(ws[1]).astype(np.float32))
    d['prev'] = {k: r.randn(*out_shape(k, g)).astype(np.float32) for k in KINDS}
    d['yact'] = r.randn(*xs).astype(np.float32)
    return d


def bias_of(kind, d):
    return {'fwd': d['b'], 'dgrad': d['bc'], 'wgrad': None}[kind]


def int_magnitude(kind, g):
    """an upper bound of sum |a| |b| + |bias| + |prev| of the integer inputs, from their ranges"""
    top = {'fwd': 3 * 2, 'dgrad': 3 * 2, 'wgrad': 3 * 3}[kind]
    return top * n_products(kind, g) + 4 + 7


def parity_class(kind, index):
    """the class of an output element, for the failure report"""
    if kind == 'dgrad':
        return "row %s (%d tap row%s), column %s" % ((("even", 1, "") if index[2] % 2 == 0 else ("odd", 2, "s"))
                                                     + ("even" if index[3] % 2 == 0 else "odd",))
    if kind == 'wgrad':
        return "tap (%d, %d): reads x rows of parity %d, columns of parity %d" % (index[2], index[3], (1 - index[2]) % 2, (1 - index[3]) % 2)
    return "output row %d reads x rows %d..%d" % (index[2], 2 * index[2] - 1, 2 * index[2] + 1)


# ---- the planners of csrc/conv_lp.hip and csrc/conv_split.hip restated (their tile and split count show in no variant
# string); the fp32 planners are read through ghm_conv2d_variant ----
def _cd(a, b):
    return (a + b - 1) // b


def _splitk(nslabs, splits):
    sps = _cd(nslabs, splits)
    return _cd(nslabs, sps), sps


def _int(env, name, default=None):
    return int(env[name]) if name in env else default


def lp_plan(g, env, cus=CUS):
    """lp_plan(N, C, Ho, Wo, K, 3, 2) -> dict(bm, tw, rt, splits, sps, grid, finish) or None"""
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    bm = 128 if (_int(env, 'GHM_LP_BM') == 128 and K >= 96) else 64
    tw = 32 if Wo % 32 == 0 else (16 if Wo % 16 == 0 else 8)
    rt = 4 if tw in (32, 16) else 2
    rows = rt * (32 // tw)
    if K < 32 or Wo % tw or Ho % rows or C % 16 or C < 16:
        return None
    grid = _cd(K, bm) * (Wo // tw) * (Ho // rows) * N
    nslabs, splits = C // 16, 1
    if grid < cus:
        splits = min(_cd(2 * cus, grid), max(nslabs // 2, 1))
    if 'GHM_LP_SPLITS' in env:
        f = int(env['GHM_LP_SPLITS'])
        splits = (f if f > 0 else 1) if f < nslabs else nslabs
    splits, sps = _splitk(nslabs, splits)
    return dict(bm=bm, tw=tw, rt=rt, splits=splits, sps=sps, grid=grid, finish=_lp_finish(splits, K, N * Ho * Wo))


def _lp_finish(splits, R, pixels):
    """which kernel ends a split-K low-precision product: sm_finish_kernel (R % 8 == 0, <= 8192 pixels) or the fp32
    igemm_splitk_epilogue (ghm_splitk_finish)"""
    if splits == 1:
        return None
    return 'sm_finish' if R % 8 == 0 and pixels <= 8192 else 'splitk_finish'


def small_map(g, kind):
    """sm_plan's map-size conditions: these products run on conv_small.hip (out of this family's scope)"""
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    HW = Ho * Wo
    CH, R = (C, K) if kind == 'fwd' else (K, C)
    if CH % 16 or CH < 16 or R % 8 or R < 8 or HW > 256 or Wo > 16:
        return False
    if not ((HW >= 64 and HW % 64 == 0 and 64 % Wo == 0) or (HW < 64 and 64 % HW == 0)):
        return False
    return N * HW <= (512 if kind == 'fwd' else 1024) and N * (HW if kind == 'fwd' else H * W) <= 8192


def lp_plan_dgrad_s2(g, env, xns=None, cus=CUS):
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    xns = C * H * W if xns is None else xns
    if Wo % 32 or K % 16 or K < 16 or C < 32 or xns % 2 or (H * W) % 2:
        return None
    tiles = [(128, 2), (64, 4), (64, 2)]
    forced = _int(env, 'GHM_LP_DGRAD_S2_TILE', -1)
    found = None
    for t in ([min(forced, 2)] if forced >= 0 else [2, 1, 0]):
        if tiles[t][0] == 128 and C < 96 and forced < 0:
            continue
        if Ho % tiles[t][1] == 0:
            found = tiles[t]
            break
    if found is None:
        return None
    bm, rt = found
    grid = _cd(C, bm) * (Wo // 32) * (Ho // rt) * N
    nslabs, splits = K // 16, 1
    if grid < cus:
        splits = min(_cd(2 * cus, grid), max(nslabs // 2, 1))
    if 'GHM_LP_DGRAD_S2_SPLITS' in env:
        splits = max(int(env['GHM_LP_DGRAD_S2_SPLITS']), 1)
    splits, sps = _splitk(nslabs, splits)
    return dict(bm=bm, rt=rt, splits=splits, sps=sps, grid=grid, finish=_lp_finish(splits, C, N * H * W))


def lp_wplan(g, env, xns=None, yns=None, cus=CUS):
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    xns, yns = C * H * W if xns is None else xns, K * Ho * Wo if yns is None else yns
    if Wo % 32 or W % 4 or K < 32 or 9 * C < 96 or xns % 4 or yns % 4 or (Ho * Wo) % 4:
        return None
    bn = 128 if K >= 96 else 64
    nseg = 2 if (Wo % 64 == 0 and 'GHM_LP_WGRAD_SEG1' not in env) else 1
    tiles = _cd(C, 128 // 9) * _cd(K, bn)
    slabs = N * Ho * (Wo // (32 * nseg))
    want = _int(env, 'GHM_LP_WGRAD_SPLITS', (2 * cus) // tiles)
    S = min(max(min(want, max(slabs // 4, 1)), 1), 1024)
    splits, sps = _splitk(slabs, S)
    return dict(bn=bn, nseg=nseg, splits=splits, sps=sps, slabs=slabs)


def sp_plan(g, env, cus=CUS):
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    tw = 32 if Wo % 32 == 0 else (16 if Wo % 16 == 0 else 8)
    if tw == 32:
        rt, waves = 4, (8 if 'GHM_SPLIT_S2_W8' in env else 4)
    else:
        rt, waves = (4 if tw == 16 else 2), 4
    rows = rt * (32 // tw)
    if K < 32 or Wo % tw or Ho % rows or C % 16 or C < 16:
        return None
    grid = _cd(K, 64) * (Wo // tw) * (Ho // rows) * N
    nslabs, splits = C // 16, 1
    if grid < cus // 2:
        splits = min(_cd(cus, grid), max(nslabs // 2, 1))
    if 'GHM_SPLIT_SPLITS' in env:
        f = int(env['GHM_SPLIT_SPLITS'])
        splits = (f if f > 0 else 1) if f < nslabs else nslabs
    splits, sps = _splitk(nslabs, splits)
    blocks = grid
    if splits == 1 and waves == 4:
        frac = float(env.get('GHM_SPLIT_PERSIST', 1.0))
        nb = int(frac * cus) // 8 * 8
        if frac > 0 and 8 <= nb < grid:
            blocks = nb
    return dict(tw=tw, rt=rt, waves=waves, splits=splits, sps=sps, grid=grid, persistent=blocks < grid,
                finish='splitk_finish' if splits > 1 else None)


def sp_plan_dgrad_s2(g, env, xns=None, cus=CUS):
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    xns = C * H * W if xns is None else xns
    if Wo % 32 or K % 16 or K < 16 or C < 32 or xns % 2 or (H * W) % 2 or Ho % 2:
        return None
    grid = _cd(C, 64) * (Wo // 32) * (Ho // 2) * N
    nslabs, splits = K // 16, 1
    if grid < cus // 2:
        splits = min(_cd(cus, grid), max(nslabs // 2, 1))
    splits, sps = _splitk(nslabs, splits)
    return dict(bm=64, rt=2, splits=splits, sps=sps, grid=grid, finish='splitk_finish' if splits > 1 else None)


def sp_wplan(g, env, cus=CUS):
    N, C, H, W, K = g
    Ho, Wo = H // 2, W // 2
    if Wo % 16 or K % 128 or C % 32:
        return None
    spx = 16 if Wo % 32 else 32
    ncols = N * (Wo // spx)
    tiles = (C // 32) * (K // 128) * ncols
    S = max(min(cus // tiles, max(Ho // 4, 1)), 1)
    rps = _cd(Ho, S)
    spc = _cd(Ho, rps)
    return dict(spx=spx, splits=ncols * spc, rows_per_split=rps, ragged=Ho % rps != 0)


def parse_variant(s):
    """'name<a, b, ...> splits=S' of ghm_conv2d_variant -> (name, [a, b, ...], S)"""
    name, rest = s.split('<', 1)
    args, tail = rest.split('>', 1)
    return name, [int(v) for v in args.split(',')], int(tail.split('splits=')[1])


# ---- the row table ----
Row = collections.namedtuple('Row', 'mode kind g view env reaches why')
VIEWS = ('whole', 'slice', 'offset')
FRONT = 1024                        # canary elements (4 KB) in front of and behind every view
OFFSET = 20                         # 'offset': the view starts 80 bytes further in (16-byte aligned, no more)
WIDER = 16                          # 'slice': channels [8, 8 + C) of a buffer of C + 16 channels (what ConcatLayer does)


def view_layout(shape, view):
    """-> (el0, nstride, total) in elements of an fp32 view of ``shape`` inside its allocation"""
    N, C, H, W = shape
    chw, hw = C * H * W, H * W
    if view == 'slice':
        ns, el0 = (C + WIDER) * hw, FRONT + 8 * hw
    elif view == 'offset':
        ns, el0 = chw, FRONT + OFFSET
    elif view == 'off4':            # four bytes in: what a vector store cannot take (tests/conv_thin_ref.py's guard rows)
        ns, el0 = chw, FRONT + 1
    else:
        assert view == 'whole'
        ns, el0 = chw, FRONT
    return el0, ns, el0 + (N - 1) * ns + chw + (8 * hw if view == 'slice' else 0) + FRONT


def strides(row):
    """(x_nstride, y_nstride) of the row's descriptor"""
    xs, _, ys = shapes(row.g)
    return view_layout(xs, row.view)[1], view_layout(ys, row.view)[1]


_F32_ROWS = [
    # forward: plan_patch(N, C, Ho, Wo, K, 3, 256, 2): 64 rows x 8 output rows, 128 x 4 under GHM_PATCH_BM; a grid under 384
    # blocks splits K when C >= 32 (C / 4 slabs, at least 4 per split)
    ('fwd', (1, 12, 16, 64, 32), 'whole', {}, dict(tile=(64, 8), splits=1), "three slabs: the single-pass form, one block"),
    ('fwd', (1, 32, 16, 64, 32), 'slice', {}, dict(tile=(64, 8), splits=2), "the base row: natural split-K + igemm_splitk_epilogue"),
    ('fwd', (3, 36, 16, 128, 48), 'offset', {}, dict(tile=(64, 8), splits=2),
     "N = 3, two column tiles, 48 filters on the 64-row tile, 9 slabs in splits of 5 + 4"),
    ('fwd', (1, 40, 8, 64, 160), 'slice', {'GHM_PATCH_BM': '128'}, dict(tile=(128, 4), splits=2),
     "the 128-row tile with 160 filters (128 + 32), Ho = 4 = one tile row, split-K"),
    ('fwd', (2, 12, 16, 64, 160), 'whole', {'GHM_PATCH_BM': '128'}, dict(tile=(128, 4), splits=1), "the 128-row tile, single pass"),
    # data gradient: dgrad_s2_plan: tiles 0 / 1 / 2 = 128 ch x 2 class rows, 64 x 4, 64 x 2 (the plan's); K / 4 slabs
    ('dgrad', (1, 32, 16, 64, 8), 'whole', {}, dict(tile=(64, 2), splits=1, dact=2), "two slabs: single pass, dact form 2"),
    ('dgrad', (1, 40, 12, 64, 32), 'slice', {'GHM_DGRAD_S2_TILE': '1'}, dict(tile=(64, 1), splits=2, dact=0),
     "the four-class-row tile on Ho = 6 (class rows rounded up), 40 channels, natural split-K"),
    ('dgrad', (3, 160, 8, 64, 12), 'offset', {'GHM_DGRAD_S2_TILE': '0'}, dict(tile=(128, 2), splits=1, dact=2),
     "the 128-channel tile with 160 channels, N = 3"),
    ('dgrad', (1, 32, 16, 128, 36), 'offset', {'GHM_DGRAD_S2_SPLITS': '2'}, dict(tile=(64, 2), splits=2, dact=0),
     "two column tiles; 9 slabs forced into 5 + 4"),
    ('dgrad', (2, 32, 8, 64, 8), 'slice', {'GHM_DGRAD_S2_TILE': '1'}, dict(tile=(64, 1), splits=1, dact=2), "tile 1 single pass, dact"),
    # weight gradient: pick_wgrad: 16-pixel slabs, at least 256 pixels per split
    ('wgrad', (1, 32, 16, 64, 32), 'whole', {}, dict(bn=32, splits=1), "256 pixels: single pass (accumulates in the kernel)"),
    ('wgrad', (3, 12, 32, 32, 48), 'offset', {'GHM_WGRAD_SPLITS': '2'}, dict(bn=64, splits=2),
     "16-column map, N = 3: two splits of 384 pixels cross the images"),
    ('wgrad', (3, 12, 32, 32, 48), 'slice', {}, dict(bn=64, splits=3), "the same with the natural three splits"),
    ('wgrad', (1, 40, 100, 32, 160), 'slice', {'GHM_WGRAD_SPLITS': '3'}, dict(bn=128, splits=3),
     "50 slabs forced into 17 + 17 + 16; 160 filters (128 + 32), 40 channels in row tiles of 14 + 14 + 12"),
]

_LP_ROWS = [
    # forward: lp_plan: 64 rows (128 under GHM_LP_BM=128 from 96 filters), 32 / 16 / 8-column tiles, C / 16 slabs
    ('fwd', (1, 32, 8, 64, 32), 'whole', {}, dict(bm=64, tw=32, splits=1), "one block"),
    ('fwd', (3, 48, 16, 128, 44), 'slice', {'GHM_LP_SPLITS': '2'}, dict(bm=64, tw=32, splits=2, finish='splitk_finish'),
     "N = 3, two column tiles, 44 filters (masked rows; K % 8 != 0: ghm_splitk_finish), 3 slabs forced into 2 + 1"),
    ('fwd', (1, 32, 16, 64, 160), 'offset', {'GHM_LP_BM': '128'}, dict(bm=128, tw=32, splits=1), "128 rows, 160 filters (128 + 32)"),
    ('fwd', (1, 16, 48, 32, 40), 'whole', {}, dict(bm=64, tw=16, splits=1), "16-column map (24 rows: not a small map), 40 filters"),
    ('fwd', (1, 64, 80, 16, 32), 'slice', {}, dict(bm=64, tw=8, splits=2, finish='sm_finish'),
     "8-column map, natural split-K finished by sm_finish_kernel"),
    # data gradient: lp_plan_dgrad_s2: tiles 0 / 1 / 2 = 128 x 2, 64 x 4, 64 x 2; Ho % rt == 0
    ('dgrad', (1, 32, 8, 64, 16), 'whole', {}, dict(tile=(64, 2), splits=1, dact=3), "Ho = 4, one slab, dact form 3"),
    ('dgrad', (1, 40, 16, 64, 32), 'slice', {'GHM_LP_DGRAD_S2_TILE': '1'}, dict(tile=(64, 4), splits=1, dact=3), "Ho = 8 on the 64 x 4 tile, 40 channels"),
    ('dgrad', (3, 160, 8, 64, 48), 'offset', {'GHM_LP_DGRAD_S2_TILE': '0', 'GHM_LP_DGRAD_S2_SPLITS': '2'},
     dict(tile=(128, 2), splits=2, dact=0, finish='sm_finish'), "128 x 2 tile with 160 channels, N = 3, 3 slabs forced into 2 + 1"),
    ('dgrad', (1, 36, 8, 128, 64), 'slice', {}, dict(tile=(64, 2), splits=2, dact=0, finish='splitk_finish'),
     "two column tiles, natural split-K; 36 channels: ghm_splitk_finish"),
    # weight gradient: lp_wplan: slabs of 32 (64 on Wo % 64 == 0) pixels of one output row, at least 4 per split
    ('wgrad', (1, 32, 8, 64, 32), 'whole', {}, dict(bn=64, nseg=1, splits=1), "4 slabs: single pass"),
    ('wgrad', (3, 16, 16, 128, 160), 'slice', {'GHM_LP_WGRAD_SPLITS': '5'}, dict(bn=128, nseg=2, splits=5),
     "64-pixel slabs, N = 3: 24 slabs forced into 5 + 5 + 5 + 5 + 4 across the images; 160 filters"),
    ('wgrad', (1, 16, 16, 128, 48), 'offset', {'GHM_LP_WGRAD_SEG1': '1'}, dict(bn=64, nseg=1, splits=4), "Wo = 64 in 32-pixel slabs, natural splits"),
]

_SP_ROWS = [
    # forward: sp_plan: 64 x 4 x 32 on four waves (eight under GHM_SPLIT_S2_W8), 16- and 8-column maps, C / 16 slabs
    ('fwd', (1, 32, 8, 64, 32), 'whole', {}, dict(tw=32, waves=4, splits=1, persistent=False), "one block"),
    ('fwd', (3, 32, 32, 128, 48), 'slice', {'GHM_SPLIT_PERSIST': '0.04'}, dict(tw=32, waves=4, splits=1, persistent=True),
     "24 tiles on 8 persistent blocks; N = 3, two column tiles, 48 filters"),
    ('fwd', (3, 32, 32, 128, 48), 'slice', {'GHM_SPLIT_PERSIST': '0'}, dict(tw=32, waves=4, splits=1, persistent=False), "the same, one tile per block"),
    ('fwd', (1, 80, 16, 64, 40), 'offset', {'GHM_SPLIT_S2_W8': '1', 'GHM_SPLIT_SPLITS': '2'}, dict(tw=32, waves=8, splits=2, persistent=False),
     "eight waves; 5 slabs forced into 3 + 2; 40 filters"),
    ('fwd', (1, 64, 8, 64, 32), 'whole', {}, dict(tw=32, waves=4, splits=2, persistent=False), "natural split-K + ghm_splitk_finish"),
    ('fwd', (1, 16, 48, 32, 32), 'offset', {}, dict(tw=16, waves=4, splits=1, persistent=False), "16-column map"),
    ('fwd', (1, 32, 80, 16, 160), 'slice', {}, dict(tw=8, waves=4, splits=1, persistent=False), "8-column map, 160 filters (64 + 64 + 32)"),
    # data gradient: sp_plan_dgrad_s2: 64 channels x 2 class rows; split-K when the grid is under 128 blocks and K >= 64
    ('dgrad', (1, 32, 8, 64, 16), 'whole', {}, dict(splits=1, dact=3), "one slab, dact"),
    ('dgrad', (3, 40, 12, 64, 32), 'slice', {}, dict(splits=1, dact=3), "Ho = 6, 40 channels, N = 3"),
    ('dgrad', (1, 64, 16, 64, 64), 'offset', {}, dict(splits=2, dact=0), "natural split-K + ghm_splitk_finish"),
    ('dgrad', (1, 160, 4, 128, 48), 'slice', {}, dict(splits=1, dact=3), "160 channels (64 + 64 + 32), two column tiles, Ho = 2"),
    # weight gradient: sp_wplan: strips of 32 (16 on 16-column maps) columns per image, split by output rows
    ('wgrad', (1, 32, 8, 64, 128), 'whole', {}, dict(spx=32, splits=1), "Ho = 4: one split (accumulates in the kernel)"),
    ('wgrad', (3, 64, 28, 32, 128), 'slice', {}, dict(spx=16, splits=9), "16-column map, N = 3: 3 strips x rows 5 + 5 + 4"),
    ('wgrad', (2, 32, 16, 128, 256), 'offset', {}, dict(spx=32, splits=8), "four strips x two row splits, two filter tiles"),
]


def _rows():
    out = [Row('f32', *r) for r in _F32_ROWS]
    out += [Row(m, *r) for m in ('bf16', 'f16') for r in _LP_ROWS]
    out += [Row(m, *r) for m in ('bf16x3', 'bf16x2') for r in _SP_ROWS]
    return out


ROWS = _rows()


def row_id(r):
    return "%s-%s-%s-%s%s" % (r.mode, r.kind, "x".join(str(v) for v in r.g), r.view,
                              "".join("-%s=%s" % (k.replace('GHM_', ''), v) for k, v in sorted(r.env.items())))


# q operands: two rows per mode, single-pass plans only: (kind, g, view of the q tensors)
Q_ROWS = [(m, k, g, v) for m in ('bf16', 'f16', 'bf16x3', 'bf16x2')
          for k, g, v in (('fwd', (2, 32, 8, 64, 48), 'slice'), ('dgrad', (2, 40, 8, 64, 32), 'whole'))]

# what the table must reach (asserted by tests/test_conv_s2_ref.py from the rows' checked claims): (family, kind, tile, splits > 1)
COVERAGE = {
    ('f32', 'fwd', (64, 8), False), ('f32', 'fwd', (64, 8), True), ('f32', 'fwd', (128, 4), False), ('f32', 'fwd', (128, 4), True),
    ('f32', 'dgrad', (64, 2), False), ('f32', 'dgrad', (64, 2), True), ('f32', 'dgrad', (64, 1), False), ('f32', 'dgrad', (64, 1), True),
    ('f32', 'dgrad', (128, 2), False), ('f32', 'wgrad', 32, False), ('f32', 'wgrad', 64, True), ('f32', 'wgrad', 128, True),
    ('lp', 'fwd', (64, 32), False), ('lp', 'fwd', (64, 32), True), ('lp', 'fwd', (128, 32), False), ('lp', 'fwd', (64, 16), False),
    ('lp', 'fwd', (64, 8), True), ('lp', 'dgrad', (64, 2), False), ('lp', 'dgrad', (64, 2), True), ('lp', 'dgrad', (64, 4), False),
    ('lp', 'dgrad', (128, 2), True), ('lp', 'wgrad', (64, 1), False), ('lp', 'wgrad', (64, 1), True), ('lp', 'wgrad', (128, 2), True),
    ('split', 'fwd', (32, 4, False), False), ('split', 'fwd', (32, 4, True), False), ('split', 'fwd', (32, 8, False), True),
    ('split', 'fwd', (32, 4, False), True), ('split', 'fwd', (16, 4, False), False), ('split', 'fwd', (8, 4, False), False),
    ('split', 'dgrad', (64, 2), False), ('split', 'dgrad', (64, 2), True), ('split', 'wgrad', 32, False), ('split', 'wgrad', 32, True),
    ('split', 'wgrad', 16, True),
}


def family(mode):
    return 'f32' if mode == 'f32' else ('lp' if mode in ('bf16', 'f16') else 'split')
