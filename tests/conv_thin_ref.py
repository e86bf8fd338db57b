"""Float64 definitions, inputs, row table and bounds of the thin first- and last-layer convolutions of csrc/conv_thin.hip
(<= 4 channels on one side, full-resolution maps), shared by tests/test_conv_thin_ref.py (CPU: validates the reference, the
inputs, the rows' claims, measures the bound and shows what the per-element checks see) and tests/test_gpu_conv_thin.py (GPU).
numpy only; built on oracle/ops.py.

Geometry g = (N, C, H, W, K, k, stride, pad):  y[n, f, i, j] = b[f] + sum_{c, a, b} xpad[n, c, s i + a, s j + b] Wc[f, c, a, b],
Wc the flipped filter (Lasagne's true convolution); the data gradient is its adjoint (+ a bias per INPUT channel, the epilogue
bias of the data-gradient entry points), the weight gradient the gradient of W.

Per-element bound of every product:  |got - ref| <= k 2^-24 M.
  ref  the float64 product of the fp32 operands;
  M    the same product of the absolute values, + |bias|;
  k    K_BOUND[(kernel family, kind)]: twice the worst of ``restate32`` over the real-input rows of that family, rounded up --
       measured against this reference, never from a kernel.  Whatever is measured, k <= n + S + 2 (n products per output, S
       partial sums): the forward error bound of an fp32 sum in any order.

restate32, forward and data gradients: every product rounded to fp32, ONE strictly sequential fp32 accumulator (np.cumsum) over
the taps and channels of an output, then the bias.  The kernels sum in MFMA blocks of two products (fanout, fanin_s1's S planes),
in T shifted planes (fanin_s1's second phase) or by fmaf in one accumulator per output parity (fanin_s2): each at least as
favourable as one sequential accumulator, hence the factor 2.

restate32, weight gradient: one sequential fp32 accumulator per big-tensor row of Wb pixels, then one sequential accumulator
over the N * Hb row sums.  This is no more favourable than thin_wgrad_kernel: there an accumulator (one MFMA wave's, per
output) adds an EIGHTH of each tile's pixels of the block's rows (PXC / 8 = 16 or 8 consecutive pixels per tile, two per
MFMA), i.e. at most rows_per_block * Wb / 8 terms in sequence where the restatement puts Wb; the block then adds its 8 wave
partials pairwise (3 levels) and ghm_reduce_splits adds at most num_cu block partials in 4 or 8 interleaved accumulators --
fewer terms per accumulator and shallower final sums than the restatement's N * Hb sequential row sums (96 .. 520 here against
at most 256 block partials in >= 4 chains).  The restatement's running sums are therefore at least as long at every level.
The restatement is evaluated on a sample: forward / data gradient on every border class and corner, the first and last row of
every image and SAMPLE random outputs; weight gradient on the corner, edge and centre taps of the first and last thin channel,
for every big channel.
"""
import collections

import numpy as np

from oracle import ops as O
from tests.conv_s2_ref import FRONT, OFFSET, WIDER, _signed, hash_g, view_layout  # noqa: F401  (the layouts of the older module; 'off4': 4 bytes in)
from tests.elementwise_q_ref import U, pieces, rel, worst  # noqa: F401  (re-exported for the two test modules)

SLOPE = 0.25                        # the activation slope of the integer pass: exact
REL_L2 = 1e-5                       # the bound of the older tests (tests/test_gpu_ops.py::test_thin_layer_kernels)
CUS = 256                           # the CU count the host-only queries plan with, and the MI355X's
SAMPLE = 4096
KIND_CODE = {'fwd': 0, 'dgrad': 1, 'wgrad': 2, 'dgrad_t': 3}
Q_MODES = ('bf16', 'f16', 'bf16x3', 'bf16x2')

# ---- the frozen k per (kernel family, kind): 2 x the worst of restate32 over the family's real-input rows (in the comment),
# rounded up.  tests/test_conv_thin_ref.py re-measures and asserts that these are exactly that.  ('dgrad_t' is held to
# 'dgrad': the same product; the pooled rows to ('fanout', 'fwd'): |max a_i - max b_i| <= max |a_i - b_i|, M the window's
# largest) ----
K_BOUND = {
    ('fanout', 'fwd'): 8, ('fanout', 'dgrad'): 5,               # 3.75  2.02
    ('fanin_s1', 'fwd'): 12, ('fanin_s1', 'dgrad'): 13,         # 5.72  6.06
    ('fanin_s2', 'dgrad'): 11,                                  # 5.10
    ('thin_wgrad', 'wgrad'): 2,                                 # 0.54
}
# (the weight gradient's M sums 3e4 .. 1.3e5 pixel products whose signs cancel in the value but not in its rounding errors'
# random walk: the worst error of the row-by-row restatement stays near half a unit of 2^-24 M.  That small k is what lets
# the check see a single missing row at a strength the norm lets through: tests/test_conv_thin_ref.py, case (c).)


def gfull(g):
    """(N, C, H, W, K, k) of a pooled row -> the stride-1 'same' geometry"""
    return tuple(g) if len(g) == 8 else tuple(g) + (1, g[5] // 2)


def out_hw(g):
    N, C, H, W, K, k, s, pad = g
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def shapes(g):
    N, C, H, W, K, k, s, pad = g
    Ho, Wo = out_hw(g)
    return (N, C, H, W), (K, C, k, k), (N, K, Ho, Wo)


def base_kind(kind):
    return {'dgrad_t': 'dgrad', 'pool': 'fwd'}.get(kind, kind)


def out_shape(kind, g):
    xs, ws, ys = shapes(g)
    if kind == 'pool':
        return ys[:2] + (ys[2] // 2, ys[3] // 2)
    return {'fwd': ys, 'dgrad': xs, 'wgrad': ws}[base_kind(kind)]


def n_products(kind, g):
    """the products of one output that are not structurally zero (stride 2: a data-gradient element meets ceil(k / 2)^2 taps
    at most)"""
    N, C, H, W, K, k, s, pad = g
    Ho, Wo = out_hw(g)
    kind = base_kind(kind)
    return {'fwd': k * k * C, 'dgrad': ((k + s - 1) // s) ** 2 * K, 'wgrad': N * Ho * Wo}[kind]


# ---- reference ----
def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def ref(kind, g, x, W, b, dy):
    """float64: 'fwd' conv(x, W) + b; 'dgrad' conv^T(dy, W) + b (b per input channel); 'wgrad' the gradient of W.  b None:
    no bias"""
    N, C, H, Wd, K, k, s, pad = g
    x, W, b, dy = _f64(x), _f64(W), _f64(b), _f64(dy)
    kind = base_kind(kind)
    if kind == 'fwd':
        y = O.corr2d_fwd(x, W[:, :, ::-1, ::-1], s, pad)
        return y if b is None else y + b[None, :, None, None]
    if kind == 'dgrad':
        dx = O.corr2d_bwd_input(dy, W[:, :, ::-1, ::-1], s, pad, H, Wd)
        return dx if b is None else dx + b[None, :, None, None]
    assert kind == 'wgrad'
    return np.ascontiguousarray(O.corr2d_bwd_weight(x, dy, s, pad, k, k)[:, :, ::-1, ::-1])


def M(kind, g, x, W, b, dy):
    """sum |a| |b| + |bias| in float64"""
    ab = lambda a: None if a is None else np.abs(_f64(a))
    return ref(kind, g, ab(x), ab(W), ab(b), ab(dy))


def act64(v, act):
    if act == 'relu':
        return np.where(v > 0, v, 0.0)
    return v if act == 'linear' else np.where(v > 0, v, SLOPE * v)


def pool_ref(y):
    """-> (pooled, mask) of a full-resolution activation: the 2x2 maximum and the mask byte of csrc/conv_thin.hip: bit
    2 dr + dc for every element of the window equal to the maximum (all ties set), GHM_POOL_SIGN = 16 where it is positive"""
    N, K, H, W = y.shape
    w = y.reshape(N, K, H // 2, 2, W // 2, 2)
    m = w.max(axis=(3, 5))
    mask = np.zeros(m.shape, np.uint8)
    for dr in range(2):
        for dc in range(2):
            mask |= ((w[:, :, :, dr, :, dc] == m) << (2 * dr + dc)).astype(np.uint8)
    mask |= ((m > 0) << 4).astype(np.uint8)
    return m, mask


# ---- the products as explicit dot products at chosen outputs (forward and data gradient) ----
def terms(kind, g, A, B, idx):
    """-> (a, b) of shape [len(idx), n]: out[idx[e]] = sum_t a[e, t] b[e, t] (taps on padding or off the stride grid are zero
    terms).  'fwd': A = x, B = W, idx (n, f, i, j), order (c, a, b); 'dgrad': A = dy, B = W, idx (n, c, h, w), order (f, a, b)"""
    N, C, H, Wd, K, k, s, pad = g
    A, B, idx = np.asarray(A), np.asarray(B), np.asarray(idx)
    E, ar = len(idx), np.arange(k)
    Wc = B[:, :, ::-1, ::-1]
    if base_kind(kind) == 'fwd':
        xp = np.pad(A, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        n, f, i, j = idx.T
        rows = (s * i)[:, None, None] + ar[None, :, None]
        cols = (s * j)[:, None, None] + ar[None, None, :]
        a = xp[n[:, None, None, None], np.arange(C)[None, :, None, None], rows[:, None], cols[:, None]]
        return a.reshape(E, -1), Wc[f].reshape(E, -1)
    assert base_kind(kind) == 'dgrad'
    Ho, Wo = out_hw(g)
    dyd = np.zeros((N, K, s * Ho + 2 * k, s * Wo + 2 * k), A.dtype)     # dyd[k + s i] = dy[i], zero elsewhere
    dyd[:, :, k:k + s * Ho:s, k:k + s * Wo:s] = A
    n, c, h, w = idx.T
    rows = (h + pad + k)[:, None, None] - ar[None, :, None]             # dy row (h + pad - a) / s where that is whole
    cols = (w + pad + k)[:, None, None] - ar[None, None, :]
    a = dyd[n[:, None, None, None], np.arange(K)[None, :, None, None], rows[:, None], cols[:, None]]
    return a.reshape(E, -1), Wc[:, c].transpose(1, 0, 2, 3).reshape(E, -1)


def sample_idx(kind, g, salt=0, count=SAMPLE):
    """output indices of a forward / data gradient: every combination of {0, 1, last - 1, last} over the four axes, the first
    and last row of every image (first and last channel, every column) and ``count`` random ones"""
    shp = out_shape(base_kind(kind), g)
    edge = [sorted({0, min(1, s - 1), max(s - 2, 0), s - 1}) for s in shp]
    grid = np.stack(np.meshgrid(*edge, indexing='ij'), -1).reshape(-1, 4)
    rows = np.stack(np.meshgrid(np.arange(shp[0]), sorted({0, shp[1] - 1}), [0, shp[2] - 1], np.arange(shp[3]), indexing='ij'), -1).reshape(-1, 4)
    r = np.random.RandomState((hash_g(g) + 17 * salt + 5) % (2 ** 31))
    rnd = np.stack([r.randint(0, s, count) for s in shp], -1)
    return np.concatenate([grid, rows, rnd])


def at(a, idx):
    idx = np.asarray(idx)
    return np.asarray(a)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


def restate32(kind, g, x, W, b, dy, idx):
    """forward / data gradient in fp32 numpy at the outputs ``idx``: rounded products, ONE sequential accumulator, the bias"""
    A = x if base_kind(kind) == 'fwd' else dy
    ta, tb = terms(kind, g, np.asarray(A, np.float32), np.asarray(W, np.float32), idx)
    acc = np.cumsum(ta * tb, axis=1, dtype=np.float32)[:, -1]
    if b is not None:
        acc = (acc + np.asarray(b, np.float32)[np.asarray(idx)[:, 1]]).astype(np.float32)
    return acc


# ---- the weight gradient, tap by tap ----
def wgrad_side(g):
    """1: the input channels are thin (big = dy on the output grid), 2: the filters are (big = x; stride 1, 'same')"""
    return 1 if g[1] <= 4 else 2


def wgrad_taps(g):
    """the sampled (thin channel, a, b) of the correlation gradient dWc: corner, edge and centre taps of the first and last thin
    channel"""
    N, C, H, W, K, k, s, pad = g
    thin = C if wgrad_side(g) == 1 else K
    ab = sorted({0, k // 2, k - 1})
    return [(t, a, b) for t in sorted({0, thin - 1}) for a in ab for b in ab]


def wgrad_planes(g, x, dy, tap):
    """-> (big [N, CB, Hb, Wb], thin plane [N, Hb, Wb]) with dWc[., tap] = sum_{n, h, w} big[n, :, h, w] plane[n, h, w]"""
    N, C, H, W, K, k, s, pad = g
    t, a, b = tap
    if wgrad_side(g) == 1:
        Ho, Wo = out_hw(g)
        xp = np.pad(x[:, t], ((0, 0), (pad, pad), (pad, pad)))
        return dy, xp[:, a:a + s * Ho:s, b:b + s * Wo:s]
    dyp = np.pad(dy[:, t], ((0, 0), (k, k), (k, k)))            # x[h, w] meets dy[h - a + pad, w - b + pad]
    return x, dyp[:, k - a + pad:k - a + pad + H, k - b + pad:k - b + pad + W]


def wgrad_index(g, tap):
    """where dWc[., tap] lies in dW[K, C, k, k] (the flipped filter): an index tuple over the big channels"""
    k = g[5]
    t, a, b = tap
    return (slice(None), t, k - 1 - a, k - 1 - b) if wgrad_side(g) == 1 else (t, slice(None), k - 1 - a, k - 1 - b)


def wgrad_at(g, x, dy, tap, dtype=np.float64, absolute=False):
    """dWc[., tap] for every big channel: float64 (the reference; ``absolute``: M), or float32 = restate32: a sequential
    accumulator per big row of Wb pixels, then one over the N * Hb row sums"""
    big, plane = wgrad_planes(g, np.asarray(x), np.asarray(dy), tap)
    if dtype == np.float64:
        big, plane = big.astype(np.float64), plane.astype(np.float64)
        if absolute:
            big, plane = np.abs(big), np.abs(plane)
        return np.einsum('nchw,nhw->c', big, plane)
    p = np.asarray(big, np.float32) * np.asarray(plane, np.float32)[:, None]
    rows = np.cumsum(p, axis=3, dtype=np.float32)[..., -1]                                  # [N, CB, Hb]
    rows = np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(rows.shape[1], -1)         # [CB, N * Hb]
    return np.cumsum(rows, axis=1, dtype=np.float32)[:, -1]


# ---- inputs ----
def int_inputs(g, salt=0):
    """x, dy in +-{1, 2, 3}, W in +-{1, 2}, integer biases and previous values: every partial sum in any order stays below
    2^24 (the weight gradients sum up to 1.4e5 pixel products of at most 9), so every kernel must return the float64 answer
    bit for bit"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt) % (2 ** 31))
    d = dict(x=_signed(r, 3, xs), W=_signed(r, 2, ws), dy=_signed(r, 3, ys), b=_signed(r, 4, ws[0]), bc=_signed(r, 4, ws[1]))
    d['prev'] = {k: _signed(r, 7, out_shape(k, g)) for k in ('fwd', 'dgrad', 'wgrad')}
    return d


def real_inputs(g, salt=0):
    """randn with per-(sample, channel) scales exp(randn): the scaled draws of tests/conv_s2_ref.py"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + salt + 1000) % (2 ** 31))
    d = dict(x=(r.randn(*xs) * np.exp(r.randn(xs[0], xs[1], 1, 1))).astype(np.float32),
             W=(r.randn(*ws) / np.sqrt(float(ws[1] * ws[2] * ws[3]))).astype(np.float32),
             dy=(r.randn(*ys) * np.exp(r.randn(ys[0], ys[1], 1, 1))).astype(np.float32),
             b=r.randn(ws[0]).astype(np.float32), bc=r.randn(ws[1]).astype(np.float32))
    d['prev'] = {k: r.randn(*out_shape(k, g)).astype(np.float32) for k in ('fwd', 'dgrad', 'wgrad')}
    return d


def bias_of(kind, d):
    return {'fwd': d['b'], 'dgrad': d['bc'], 'wgrad': None}[base_kind(kind)]


def int_magnitude(kind, g):
    """an upper bound of sum |a| |b| + |bias| + |prev| of the integer inputs, from their ranges"""
    top = {'fwd': 3 * 2, 'dgrad': 3 * 2, 'wgrad': 3 * 3}[base_kind(kind)]
    return top * n_products(kind, g) + 4 + 7


def border_class(kind, g, index):
    """the class of an output element, for the failure report"""
    shp = out_shape(kind, g)
    if base_kind(kind) == 'wgrad':
        return "tap (%d, %d) of filter %d, channel %d" % (index[2], index[3], index[0], index[1])
    edge = lambda v, n: "first" if v == 0 else ("last" if v == n - 1 else "inner")
    return "sample %d, %s row, %s column" % (index[0], edge(index[2], shp[2]), edge(index[3], shp[3]))


# ---- the planners of csrc/conv_thin.hip restated (the plan shows in no variant string) ----
def fanout_plan(rows_out, thin_ch, k, stride, Hout, Wout, env=None):
    """fanout_plan + fanout_geometry_ok + launch_fanout's template choice -> dict(KSTEPS, R, NS, RPI, KRT, LW, GPR) or None"""
    env = env or {}
    Q = thin_ch * k * k
    if not (Q <= 36 and (rows_out == 64 or (rows_out == 128 and Q <= 12))):
        return None
    NS = 4 if rows_out <= 64 else 2
    gpr = Wout // (NS * 32)
    rpi = 1 if gpr >= 4 else (4 + gpr - 1) // (gpr if gpr > 0 else 1)
    if int(env.get('GHM_FANOUT_RPI', 0)) > 0:
        rpi = int(env['GHM_FANOUT_RPI'])
    while rpi > 1 and Hout % rpi != 0:
        rpi -= 1
    KRT, LW = k + (rpi - 1) * stride, (((Wout - 1) * stride + k) + 63) & ~63
    if Wout % (NS * 32) or 2 * thin_ch * KRT * LW * 4 + 2048 > 150 * 1024:
        return None
    ks = (Q + 1) // 2
    KSTEPS = 6 if rows_out == 128 else (5 if ks <= 5 else (13 if ks <= 13 else 18))
    return dict(KSTEPS=KSTEPS, R=rows_out, NS=NS, RPI=rpi, KRT=KRT, LW=LW, GPR=gpr)


def fanout_reaches(kind, g, env=None):
    """(KSTEPS, R, NS, RPI, iterations) of a fan-out row, or None"""
    N, C, H, W, K, k, s, pad = g
    Ho, Wo = out_hw(g)
    if base_kind(kind) == 'fwd':
        if N * Ho * Wo < 32768:
            return None
        p, n_it = fanout_plan(K, C, k, s, Ho, Wo, env), N * Ho
    else:
        if s != 1 or (Ho, Wo) != (H, W) or N * H * W < 32768:
            return None
        p, n_it = fanout_plan(C, K, k, 1, H, W, env), N * H
    return None if p is None else (p['KSTEPS'], p['R'], p['NS'], p['RPI'], n_it // p['RPI'])


def pool_reaches(g, env=None):
    """(KSTEPS, WS, row pairs) of thin_fanout_fwd_pool: RPI = 2, the eight-wave form unless GHM_FANOUT_NO_SPLIT"""
    N, C, H, W, K, k, s, pad = g
    ks = (C * k * k + 1) // 2
    return (5 if ks <= 5 else (13 if ks <= 13 else 18), 1 if 'GHM_FANOUT_NO_SPLIT' in (env or {}) else 2, N * H // 2)


def wgrad_reaches(g):
    """(RB, CBQ, NC, rows) of thin_wgrad, or None"""
    N, C, H, W, K, k, s, pad = g
    Ho, Wo = out_hw(g)
    if wgrad_side(g) == 1:
        big, thin, Hb, Wb, st = K, C, Ho, Wo, s
    else:
        if s != 1 or (Ho, Wo) != (H, W):
            return None
        big, thin, Hb, Wb, st = C, K, H, W, 1
    Q = thin * k * k
    if not (big == 64 or (big == 128 and Q <= 32)) or Q > 36:
        return None
    pxc = 128 if big == 64 else 64
    LW = (((Wb - 1) * st + k) + 63) & ~63
    if Wb % pxc or Wb // pxc < 2 or N * Hb * Wb < 32768 or (3 * big * pxc + 2 * thin * k * LW) * 4 > 158 * 1024:
        return None
    return (big // 32, (Q + 31) // 32, Wb // pxc, N * Hb)


def iterations(row):
    """the persistent kernel's iteration count of a row (0: not a persistent kernel)"""
    if row.kernel in ('fanout', 'pool', 'thin_wgrad'):
        return row.reaches['plan'][-1]
    return 0


# ---- the row table ----
Row = collections.namedtuple('Row', 'kernel kind g view env reaches why')
VIEWS = ('whole', 'slice', 'offset')


def strides(row):
    """(x_nstride, y_nstride) of the row's descriptor"""
    xs, _, ys = shapes(row.g)
    return view_layout(xs, row.view)[1], view_layout(ys, row.view)[1]


RPI1 = {'GHM_FANOUT_RPI': '1'}


def _fo(kind, g, view, env, plan, why):
    v = {'fwd': 'fanout_kernel<fwd>', 'dgrad': 'fanout_kernel<dgrad>', 'dgrad_t': 'fanout_kernel<dgrad_t>'}[kind]
    return Row('fanout', kind, g, view, env, dict(variant=v, plan=plan), why)


def _both(g, views, plan, why):
    return [_fo('dgrad', g, views[0], {}, plan, why), _fo('dgrad_t', g, views[1], {}, plan, why + " (transposed weights, swapped descriptor)")]


def _rows():
    rows = [
        # fanout_kernel<fwd>: plan = (KSTEPS, R, NS, RPI, iterations)
        _fo('fwd', (2, 1, 128, 128, 64, 5, 1, 2), 'slice', {}, (13, 64, 4, 4, 64), "d_conv1: Q 25 on KSTEPS 13 with one dead reduction row"),
        _fo('fwd', (2, 4, 256, 256, 64, 3, 2, 1), 'offset', {}, (18, 64, 4, 4, 64), "pd_conv1: Q 36, stride-2 staging, LW 320"),
        _fo('fwd', (2, 1, 256, 256, 64, 3, 2, 1), 'whole', {}, (5, 64, 4, 4, 64), "the U-Net's conv1: KSTEPS 5"),
        _fo('fwd', (1, 3, 128, 256, 64, 3, 1, 1), 'slice', {}, (18, 64, 4, 2, 64), "Q 27 on KSTEPS 18 with nine dead rows, RPI 2"),
        _fo('fwd', (2, 3, 256, 256, 128, 2, 2, 0), 'slice', {}, (6, 128, 2, 2, 128), "the final deconv's data gradient form: R 128, NS 2"),
        _fo('fwd', (1, 1, 64, 512, 64, 5, 1, 2), 'offset', {}, (13, 64, 4, 1, 64), "four groups per row, RPI 1"),
        _fo('fwd', (1, 1, 96, 384, 64, 5, 1, 2), 'whole', {}, (13, 64, 4, 2, 48), "three groups per row: six groups on four waves, a ragged group loop"),
        _fo('fwd', (2, 1, 130, 128, 64, 5, 1, 2), 'offset', {}, (13, 64, 4, 2, 130), "RPI falls back from 4 to 2: 130 % 4 and 130 % 3 are non-zero"),
        # more than one iteration per persistent block
        _fo('fwd', (5, 1, 104, 128, 64, 5, 1, 2), 'slice', RPI1, (13, 64, 4, 1, 520), "520 iterations: some blocks run three, both LDS buffers reused"),
        _fo('fwd', (5, 1, 104, 128, 64, 5, 1, 2), 'slice', {}, (13, 64, 4, 4, 130), "the control of the row above: one iteration per block"),
        _fo('dgrad', (5, 64, 104, 128, 1, 5, 1, 2), 'offset', RPI1, (13, 64, 4, 1, 520), "520 iterations of the data gradient"),
    ]
    rows += _both((2, 64, 128, 128, 1, 5, 1, 2), ('slice', 'offset'), (13, 64, 4, 4, 64), "g_out")
    rows += _both((1, 64, 128, 256, 3, 3, 1, 1), ('whole', 'slice'), (18, 64, 4, 2, 64), "three filters: Q 27")
    rows += _both((2, 128, 128, 128, 1, 3, 1, 1), ('offset', 'whole'), (6, 128, 2, 2, 128), "R 128, Q 9")
    s1 = lambda kind, g, view, form, why: Row('fanin_s1', kind, g, view, {}, dict(variant='fanin_s1_kernel<%s>' % kind, form=form), why)
    rows += [
        # fanin_s1_kernel: form = (k, big channels)
        s1('fwd', (2, 64, 128, 128, 1, 5, 1, 2), 'slice', (5, 64), "g_out (and its tanh)"),
        s1('fwd', (2, 128, 64, 256, 3, 3, 1, 1), 'offset', (3, 128), "27 of 32 rows live"),
        s1('fwd', (2, 128, 128, 128, 1, 5, 1, 2), 'whole', (5, 128), "128 channels"),
        s1('fwd', (1, 64, 128, 256, 1, 3, 1, 1), 'offset', (3, 64), "3x3, 64 channels"),
        s1('dgrad', (2, 1, 128, 128, 64, 5, 1, 2), 'slice', (5, 64), "d_conv1's data gradient"),
        s1('dgrad', (1, 3, 128, 256, 64, 3, 1, 1), 'whole', (3, 64), "three channels x nine taps"),
        s1('dgrad', (2, 1, 128, 128, 128, 5, 1, 2), 'offset', (5, 128), "128 filters"),
    ]
    s2 = lambda g, view, why: Row('fanin_s2', 'dgrad', g, view, {}, dict(variant='fanin_s2_kernel<%d>' % g[5], form=(g[5], g[1])), why)
    rows += [
        # fanin_s2_kernel: form = (k, thin channels)
        s2((1, 4, 256, 256, 64, 3, 2, 1), 'slice', "pd_conv1"),
        s2((1, 1, 260, 254, 40, 3, 2, 1), 'offset', "P = 130 * 127 = 16510: a ragged last block, odd Wo, 40 filters"),
        s2((2, 3, 192, 192, 256, 3, 2, 1), 'slice', "256 filters: the LDS limit; N = 2 in a slice"),
        s2((2, 3, 256, 128, 128, 2, 2, 0), 'whole', "the final Deconv2DLayer"),
        s2((1, 1, 260, 254, 24, 2, 2, 0), 'offset', "k2, ragged last block, odd Wo"),
        s2((1, 4, 256, 256, 64, 2, 2, 0), 'slice', "k2, four channels"),
    ]
    wg = lambda g, view, plan, why: Row('thin_wgrad', 'wgrad', g, view, {}, dict(variant='thin_wgrad_kernel<%d>' % (g[4] if g[1] <= 4 else g[1]),
                                                                               plan=plan, side=1 if g[1] <= 4 else 2), why)
    rows += [
        # thin_wgrad_kernel: plan = (RB, CBQ, NC, rows)
        wg((1, 1, 128, 256, 64, 5, 1, 2), 'whole', (2, 1, 2, 128), "<2, 1>, NC 2, one row per block"),
        wg((1, 4, 256, 512, 64, 3, 2, 1), 'offset', (2, 2, 2, 128), "<2, 2>: Q 36, stride-2 thin rows"),
        wg((2, 3, 256, 256, 128, 2, 2, 0), 'slice', (4, 1, 2, 256), "<4, 1>; N = 2 in a slice"),
        wg((1, 1, 96, 384, 64, 5, 1, 2), 'slice', (2, 1, 3, 96), "NC 3: the three-tile ring wraps mid-row"),
        wg((1, 64, 128, 256, 1, 5, 1, 2), 'offset', (2, 1, 2, 128), "filter side: g_out's weight gradient, taps negated"),
        wg((2, 128, 128, 128, 3, 3, 1, 1), 'slice', (4, 1, 2, 256), "filter side, 128 channels, Q 27"),
        wg((5, 1, 104, 256, 64, 5, 1, 2), 'slice', (2, 1, 2, 520), "520 rows: blocks 0..7 take three rows, the rest two"),
        wg((3, 1, 96, 256, 64, 5, 1, 2), 'whole', (2, 1, 2, 288), "288 rows: some blocks two, some one"),
    ]
    po = lambda g, view, env, plan, why: Row('pool', 'pool', gfull(g), view, env, dict(variant='pool', plan=plan), why)
    nosplit = {'GHM_FANOUT_NO_SPLIT': '1'}
    rows += [
        # the pooled fan-out forward: plan = (KSTEPS, WS, row pairs)
        po((8, 1, 64, 64, 64, 5), 'slice', {}, (13, 2, 256), "d_conv1 + LeakyRectify + MaxPool2D, eight waves"),
        po((8, 1, 64, 64, 64, 5), 'offset', nosplit, (13, 1, 256), "the same on four waves"),
        po((2, 4, 128, 128, 64, 3), 'offset', {}, (18, 2, 128), "four channels, Q 36, eight waves"),
        po((2, 4, 128, 128, 64, 3), 'slice', nosplit, (18, 1, 128), "the same on four waves"),
        po((5, 1, 208, 128, 64, 5), 'whole', {}, (13, 2, 520), "520 row pairs: some blocks run three"),
    ]
    return rows


ROWS = _rows()
# rows whose persistent blocks must run more than one iteration: row id -> the multiple of the CU count the count exceeds
MULTI = {('fanout', 'fwd', (5, 1, 104, 128, 64, 5, 1, 2), True): 2, ('fanout', 'dgrad', (5, 64, 104, 128, 1, 5, 1, 2), True): 2,
         ('pool', 'pool', (5, 1, 208, 128, 64, 5, 1, 2), False): 2, ('thin_wgrad', 'wgrad', (5, 1, 104, 256, 64, 5, 1, 2), False): 2,
         ('thin_wgrad', 'wgrad', (3, 1, 96, 256, 64, 5, 1, 2), False): 1}


def multi_key(r):
    return (r.kernel, r.kind, r.g, bool(r.env))


def row_id(r):
    return "%s-%s-%s-%s%s" % (r.kernel, r.kind, "x".join(str(v) for v in r.g), r.view,
                              "".join("-%s=%s" % (k.replace('GHM_', ''), v) for k, v in sorted(r.env.items())))


# q epilogue: three fan-out forward rows (KSTEPS 5, 13, 18) and the pooled rows that thin_fanout_fwd_pool serves with a q
# copy (up to 26 reduction rows, eight waves), each in a 'slice' and an 'offset' q view.  In 'bf16' / 'f16' thin_pool_lp
# (csrc/conv_thin_lp.hip) would take the pooled call: out of scope here, so those run under GHM_NO_THIN_LP=1
Q_ROWS = [('fwd', (2, 1, 256, 256, 64, 3, 2, 1), 5), ('fwd', (2, 1, 128, 128, 64, 5, 1, 2), 13), ('fwd', (2, 4, 256, 256, 64, 3, 2, 1), 18),
          ('pool', (8, 1, 64, 64, 64, 5, 1, 2), 13), ('pool', (5, 1, 208, 128, 64, 5, 1, 2), 13)]
Q_ENV = {'GHM_NO_THIN_LP': '1'}

# the alignment guard: one row per entry point, the output view 4 bytes in: (entry point, g, the general kernel that takes it)
MISALIGNED = [('fwd', (2, 1, 128, 128, 64, 5, 1, 2)), ('dgrad', (2, 64, 128, 128, 1, 5, 1, 2)), ('dgrad_t', (2, 64, 128, 128, 1, 5, 1, 2)),
              ('pool', (8, 1, 64, 64, 64, 5, 1, 2))]

# every instantiation the table must reach (asserted by tests/test_conv_thin_ref.py from the rows' checked claims); the ACC
# forms are reached by the accumulate calls of every fan-out row, QOUT by Q_ROWS
COVERAGE = (
    {('fanout', ks, form) for ks in (5, 13, 18) for form in ('plain', 'ACC', 'QOUT')} | {('fanout', 6, 'plain'), ('fanout', 6, 'ACC')}
    | {('pool', 'WS1'), ('pool', 'WS2'), ('pool', 'QOUT')}
    | {('fanin_s1', k, ch) for k in (5, 3) for ch in (64, 128)}
    | {('fanin_s2', k, c) for k in (3, 2) for c in (1, 3, 4)}
    | {('thin_wgrad', 2, 1), ('thin_wgrad', 2, 2), ('thin_wgrad', 4, 1), ('thin_wgrad', 'side', 1), ('thin_wgrad', 'side', 2)}
)


def family_key(row):
    return (row.kernel if row.kernel != 'pool' else 'fanout', base_kind(row.kind))
