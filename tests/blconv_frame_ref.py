"""Frame-only float64 definitions, fp32 restatements of the intermediate buffers, the split plan, the row table, inputs and
bounds of the border ("frame") term of BilinearUpsample2DLayer(2) -> 3x3 'same' convolution (csrc/conv_bilinear.hip), shared
by tests/test_blconv_frame_ref.py (CPU: validates the definitions, the rows' claims, the inputs and measures the bound) and
tests/test_gpu_blconv_frame.py (GPU).  numpy only; built on oracle/ops.py.

Geometry g = (N, C, K, n1, n2): coarse input x [N, C, n1, n2], fine output 2 n1 x 2 n2, held parity-planar [N, 4K, n1, n2] with
channel (2 p + q) K + k for the fine pixel (2 a + p, 2 b + q).  The frame F = U x U^T - U0 x U0^T (oracle.ops.bilinear_conv_frame)
lives on fine rows -1, 2 n1 - 1 and columns -1, 2 n2 - 1; its valid 3x3 correlation with the flipped filter touches the fine
output rows {0, 2 n1 - 2, 2 n1 - 1} and columns {0, 2 n2 - 2, 2 n2 - 1} only.

Per-element bound of every product:  |got - ref| <= k 2^-24 M.
  ref  the float64 frame-only result (+ the previous value: all three entry points add onto their destination);
  M    the same computation with every operand and every coefficient (the frame's -1/2 included) replaced by its absolute
       value, + |previous|;
  k    K_BOUND below: twice the worst of ``restate32`` over the real-input rows, rounded up -- measured against this reference,
       never from a kernel.  restate32 is the product in fp32 numpy from the ROUNDED fp32 line values, with rounded products
       and ONE strictly sequential fp32 accumulator (np.cumsum), then the previous value.  The kernels sum in other orders (MFMA
       blocks of two products, four waves, split partials, the six jobs, the fold's few terms): each is at least as favourable.
       Whatever is measured, ``bound`` never lets k exceed products per output + splits + 4, the forward error bound of an fp32
       sum in any order (+ 4: the rounded line value, the two jobs or lines that meet at a pixel, the previous value).
"""
import collections

import numpy as np

from oracle import ops as O
from tests.conv_s2_ref import CUS, VIEWS, hash_g, view_layout  # noqa: F401  (re-exported for the two test modules)
from tests.elementwise_q_ref import U, worst  # noqa: F401

KINDS = ('fwd', 'dgrad', 'wgrad')
SAMPLE = 512                        # outputs per row and kind on which restate32 is evaluated (+ every border class)

# ---- the frozen k per kind: 2 x the worst of restate32 over the rows (in the comment), rounded up.
# tests/test_blconv_frame_ref.py re-measures and asserts that these are exactly that ----
K_BOUND = {'fwd': 10, 'dgrad': 14, 'wgrad': 9}                    # 4.80  6.77  4.31


def shapes(g):
    """(x, W, parity-planar y) shapes"""
    N, C, K, n1, n2 = g
    return (N, C, n1, n2), (K, C, 3, 3), (N, 4 * K, n1, n2)


def out_shape(kind, g):
    xs, ws, ys = shapes(g)
    return {'fwd': ys, 'dgrad': xs, 'wgrad': ws}[kind]


def n_products(kind, g):
    """the FEWEST products any output element of the kind sums (one job of 3 C, one line position of one job, a 2 x 2 map)"""
    N, C, K, n1, n2 = g
    return {'fwd': 3 * C, 'dgrad': 6 * K, 'wgrad': 2 * N * (n1 + n2)}[kind]


def bound(kind, g, splits):
    return min(K_BOUND[kind], n_products(kind, g) + splits + 4)


# ---- parity-planar <-> fine ----
def to_pp(hi):
    N, K, H, W = hi.shape
    return np.ascontiguousarray(hi.reshape(N, K, H // 2, 2, W // 2, 2).transpose(0, 3, 5, 1, 2, 4)).reshape(N, 4 * K, H // 2, W // 2)


def to_hi(pp):
    N, K4, n1, n2 = pp.shape
    return np.ascontiguousarray(pp.reshape(N, 2, 2, K4 // 4, n1, n2).transpose(0, 3, 4, 1, 5, 2)).reshape(N, K4 // 4, 2 * n1, 2 * n2)


def fine_border(n1, n2):
    """bool [2 n1, 2 n2]: the fine output pixels the frame reaches"""
    m = np.zeros((2 * n1, 2 * n2), bool)
    m[[0, -2, -1], :] = True
    m[:, [0, -2, -1]] = True
    return m


def border_pp(g):
    """bool [N, 4K, n1, n2]: ``fine_border`` in the parity-planar tensor"""
    N, C, K, n1, n2 = g
    return to_pp(np.broadcast_to(fine_border(n1, n2), (N, K, 2 * n1, 2 * n2)))


def border_coarse(g):
    """bool [N, C, n1, n2]: the coarse pixels the frame reads and its data gradient writes"""
    N, C, K, n1, n2 = g
    m = np.zeros((n1, n2), bool)
    m[[0, -1], :] = True
    m[:, [0, -1]] = True
    return np.broadcast_to(m, (N, C, n1, n2))


# ---- the frame operator with its coefficient sign explicit (the absolute-value form gives M), and its adjoint ----
def _d_axis(v, axis, s):
    """D along ``axis``: n samples -> fine positions -1 .. 2n; (D v)[-1] = s v[0] / 2, (D v)[2n - 1] = v[n - 1] / 2 (s = -1: the
    operator; s = +1: its absolute value)"""
    v = np.moveaxis(v, axis, -1)
    n = v.shape[-1]
    out = np.zeros(v.shape[:-1] + (2 * n + 2,), v.dtype)
    out[..., 0] = s * 0.5 * v[..., 0]
    out[..., 2 * n] += 0.5 * v[..., n - 1]
    return np.moveaxis(out, -1, axis)


def _d_axis_t(g, axis, s):
    g = np.moveaxis(g, axis, -1)
    n = (g.shape[-1] - 2) // 2
    out = np.zeros(g.shape[:-1] + (n,), g.dtype)
    out[..., 0] = s * 0.5 * g[..., 0]
    out[..., n - 1] += 0.5 * g[..., 2 * n]
    return np.moveaxis(out, -1, axis)


def _u_axis_t(g, axis):
    """adjoint of oracle.ops._bl_u_axis: drop the zero ring, then Theano's operator transposed"""
    g = np.moveaxis(g, axis, -1)[..., 1:-1]
    return O._bilin_axis_vjp(np.ascontiguousarray(np.moveaxis(g, -1, axis)), axis)


def _u0_axis_t(g, axis):
    """adjoint of oracle.ops._bl_u0_axis"""
    g = np.moveaxis(g, axis, -1)
    n = (g.shape[-1] - 2) // 2
    vp = np.zeros(g.shape[:-1] + (n + 2,), g.dtype)
    vp[..., 1:] += g[..., 1::2]
    vp[..., :-1] += 0.5 * g[..., 0::2]
    vp[..., 1:] += 0.5 * g[..., 0::2]
    return np.moveaxis(vp[..., 1:-1], -1, axis)


def frame(x, s=-1.0):
    """F = (D x) U^T + U0 (x D^T) [N, C, 2 n1 + 2, 2 n2 + 2]; s = -1: oracle.ops.bilinear_conv_frame; s = +1: |F| coefficient-wise"""
    return O._bl_u_axis(_d_axis(x, 2, s), 3) + O._bl_u0_axis(_d_axis(x, 3, s), 2)


def frame_t(G, s=-1.0):
    return _d_axis_t(_u_axis_t(G, 3), 2, s) + _d_axis_t(_u0_axis_t(G, 2), 3, s)


def _f64(a):
    return np.asarray(a, np.float64)


def frame_fwd(x, W):
    """the valid 3x3 correlation of the frame of x with the flipped filter, parity-planar [N, 4K, n1, n2]"""
    return to_pp(O.corr2d_fwd(O.bilinear_conv_frame(_f64(x)), O._flip(_f64(W)), 1, 0))


def frame_dgrad(dy_pp, W):
    """the adjoint of frame_fwd in x: [N, C, n1, n2]"""
    dy = to_hi(_f64(dy_pp))
    return frame_t(O.corr2d_bwd_input(dy, O._flip(_f64(W)), 1, 0, dy.shape[2] + 2, dy.shape[3] + 2))


def frame_wgrad(x, dy_pp):
    """the adjoint of frame_fwd in W: [K, C, 3, 3]"""
    return np.ascontiguousarray(O._flip(O.corr2d_bwd_weight(O.bilinear_conv_frame(_f64(x)), to_hi(_f64(dy_pp)), 1, 0, 3, 3)))


def ref(kind, x, W, dy_pp):
    return {'fwd': lambda: frame_fwd(x, W), 'dgrad': lambda: frame_dgrad(dy_pp, W), 'wgrad': lambda: frame_wgrad(x, dy_pp)}[kind]()


def M(kind, x, W, dy_pp, prev=None):
    """the same computations with |operands| and |coefficients|, + |previous|"""
    if kind == 'fwd':
        m = to_pp(O.corr2d_fwd(frame(np.abs(_f64(x)), 1.0), np.abs(O._flip(_f64(W))), 1, 0))
    elif kind == 'dgrad':
        dy = to_hi(np.abs(_f64(dy_pp)))
        m = frame_t(O.corr2d_bwd_input(dy, np.abs(O._flip(_f64(W))), 1, 0, dy.shape[2] + 2, dy.shape[3] + 2), 1.0)
    else:
        m = np.ascontiguousarray(O._flip(O.corr2d_bwd_weight(frame(np.abs(_f64(x)), 1.0), to_hi(np.abs(_f64(dy_pp))), 1, 0, 3, 3)))
    return m if prev is None else m + np.abs(_f64(prev))


# ---- the four intermediate buffers restated in fp32 (csrc/conv_bilinear.hip's header comments give the layouts) ----
# job -> (frame line, the fixed tap index, row job?); tap (a, b) of the packed correlation taps is index 3 a + b
JOB_LINE = np.array([0, 1, 1, 2, 3, 3])
JOB_FIXED = np.array([0, 2, 1, 0, 2, 1])
JOB_TAP = np.array([[f * 3 + t if j < 3 else t * 3 + f for t in range(3)] for j, f in enumerate(JOB_FIXED)])
LINE_JOBS = ((0, -1), (1, 2), (3, -1), (4, 5))


def lp_of(n1, n2):
    return (2 * max(n1, n2) + 4 + 31) // 32 * 32


def frame_sizes(g):
    """floats of the two caller-owned allocations (ghm_blconv_frame_sizes) and the offsets of their second halves"""
    N, C, K, n1, n2 = g
    LP = lp_of(n1, n2)
    fl, dyl = N * 4 * C * LP, 6 * N * K * (LP + 32)
    return dict(LP=LP, fl=fl, flt_at=fl + 64, fl_floats=2 * (fl + 64), dyl=dyl, dylt_at=dyl, dyl_floats=2 * dyl)


def _line_u(e, LP):
    """Theano's operator with its zero ring on the last axis, array index = fine position + 1, in the dtype of ``e``"""
    n, h = e.shape[-1], e.dtype.type(0.5)
    out = np.zeros(e.shape[:-1] + (LP,), e.dtype)
    out[..., 1:1 + 2 * n:2] = e
    out[..., 2:2 + 2 * n:2] = h * (e + e[..., np.minimum(np.arange(n) + 1, n - 1)])
    return out


def _line_u0(e, LP):
    """the natural operator (e zero outside) on the last axis, fine positions -1 .. 2n at array index 0 .. 2n + 1"""
    n, h = e.shape[-1], e.dtype.type(0.5)
    z = np.zeros_like(e[..., :1])
    vp = np.concatenate([z, e, z], -1)
    out = np.zeros(e.shape[:-1] + (LP,), e.dtype)
    out[..., 1:2 * n + 2:2] = vp[..., 1:]
    out[..., 0:2 * n + 1:2] = h * (vp[..., :-1] + vp[..., 1:])
    return out


def lines(x, dtype=np.float32):
    """FL [N, 4, C, LP]: in float32 every entry is a zero, +-0.5 x, or ONE rounded 0.5 (a + b) of exact halves -- the kernel's
    bits (float64: for the check of ``terms`` against the reference)"""
    x = np.asarray(x, dtype)
    N, C, n1, n2 = x.shape
    LP, h = lp_of(n1, n2), x.dtype.type(0.5)
    return np.stack([_line_u(-h * x[:, :, 0, :], LP), _line_u(h * x[:, :, n1 - 1, :], LP),
                     _line_u0(-h * x[:, :, :, 0], LP), _line_u0(h * x[:, :, :, n2 - 1], LP)], 1)


def transposed(a):
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


def dyl(dy_pp, dtype=np.float32):
    """DYL [6, N, K, LP + 32]: the six border lines of the fine dy at array index 2 + position, zeros elsewhere"""
    hi = to_hi(np.asarray(dy_pp, dtype))
    N, K, H, W = hi.shape
    out = np.zeros((6, N, K, lp_of(H // 2, W // 2) + 32), dtype)
    for job, r in enumerate((0, H - 2, H - 1)):
        out[job, :, :, 2:2 + W] = hi[:, :, r, :]
    for job, c in enumerate((0, W - 2, W - 1)):
        out[3 + job, :, :, 2:2 + H] = hi[:, :, :, c]
    return out


# ---- the split plan of csrc/conv_bilinear.hip restated ----
def _cd(a, b):
    return (a + b - 1) // b


def bl_splits(contraction, tiles, cus):
    return max(min(_cd(4 * cus, tiles), contraction // 256, 32), 1)


def ranges(total, splits):
    """the channel (forward) / filter (data gradient) range of every split: per = ceil((total / 2) / splits) * 2"""
    per = _cd(total // 2, splits) * 2
    return [(sp * per, max(min(total, sp * per + per), sp * per)) for sp in range(splits)]


def plan(g, cus=CUS):
    N, C, K, n1, n2 = g
    nmax, nmin = max(n1, n2), min(n1, n2)
    used_f, used_d = _cd(2 * nmax, 32), _cd(2 * nmax + 2, 32)
    sf = bl_splits(3 * C, (K // 32) * used_f * 6 * N, cus)
    sd = bl_splits(6 * K, (C // 32) * used_d * 4 * N, cus)
    sw = bl_splits(2 * N * (n1 + n2), (K // 32) * (C // 32) * 9, cus)
    if sw > nmin // 4:
        sw = max(nmin // 4, 1)
    return dict(LP=lp_of(n1, n2), used=(used_f, used_d), splits=(sf, sd, sw), ranges=(ranges(C, sf), ranges(K, sd)))


def cover(g, cus=CUS):
    """the split paths a geometry reaches: {(kind, tag)}, tag a split count, '3 ragged' or '>= 8'"""
    p = plan(g, cus)
    out = set()
    for kind, s, rg in zip(KINDS, p['splits'], p['ranges'] + (None,)):
        tag = s
        if kind != 'wgrad' and s == 3:
            tag = '3 ragged' if len({hi - lo for lo, hi in rg}) > 1 else 3
        out.add((kind, '>= 8' if s >= 8 else tag))
    return out


COVERAGE = ({('fwd', t) for t in (1, 2, '3 ragged', 4, '>= 8')} | {('dgrad', t) for t in (1, 2, '3 ragged', '>= 8')}
            | {('wgrad', t) for t in (1, 2, 3)})

# ---- the row table: the smallest shapes that reach each path ----
Row = collections.namedtuple('Row', 'g splits views why')      # splits: (fwd, dgrad, wgrad) at 256 CUs; views: of (x, y, dy, dx)
_ROWS = [
    ((1, 32, 32, 2, 2), (1, 1, 1), "smallest map served: fine rows {0, 2, 3}, one middle row, fold with n1 - 2 == 0"),
    ((3, 32, 64, 2, 9), (1, 1, 1), "rectangular, odd, minimal n1, K != C"),
    ((2, 64, 32, 3, 2), (1, 1, 1), "minimal n2, C != K"),
    ((1, 32, 32, 14, 14), (1, 1, 1), "LP == 2 n + 4 == 32: the forward GEMM's 2-float over-read lands in the next row and in the 64-float pad"),
    ((1, 32, 32, 15, 15), (1, 1, 1), "data-gradient tile exactly full"),
    ((1, 32, 32, 16, 15), (1, 1, 1), "forward tile exactly full (2 n1 = 32), data gradient takes 2 tiles, lines of two lengths"),
    ((1, 192, 32, 2, 2), (2, 1, 1), "first forward split, ranges 96 / 96"),
    ((1, 256, 128, 2, 3), (3, 3, 1), "ragged ranges, 86 / 86 / 84 channels and 44 / 44 / 40 filters"),
    ((2, 352, 96, 3, 2), (4, 2, 1), "4 and 2 splits, batch 2"),
    ((1, 1024, 512, 2, 2), (11, 8, 1), "the 512-px generator's deepest bilinear stage at batch 1 (ranges 10 x 94 + 84)"),
    ((4, 1024, 512, 4, 4), (3, 2, 1), "the same stage family at batch 4"),
    ((8, 32, 32, 16, 16), (1, 1, 2), "smallest weight-gradient split"),
    ((4, 32, 32, 48, 48), (1, 1, 3), "3 splits, 3 forward and 4 data-gradient position tiles"),
    ((4, 32, 32, 12, 84), (1, 1, 3), "the npmin / 4 cap met exactly: the short part has 12 position pairs = splits x 4 waves; LP = 192"),
    ((2, 32, 32, 31, 130), (1, 1, 2), "odd and long: 9 position tiles, LP = 288"),
]
# x, y and dx take the three layouts in rotation (every row has two of them in a non-whole view); dy follows x
ROWS = [Row(g, s, (VIEWS[i % 3], VIEWS[(i + 1) % 3], VIEWS[i % 3], VIEWS[(i + 2) % 3]), why) for i, (g, s, why) in enumerate(_ROWS)]


def row_id(r):
    return "x".join(str(v) for v in r.g)


# ---- inputs, deterministic per geometry ----
def int_inputs(g):
    """x a multiple of 4 in [-16, 16] (every line value an integer of at most 8), W in [-2, 2], dy in [-3, 3], previous values in
    [-7, 7]: exact zeros and both signs everywhere, every partial sum in any order far below 2^24"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState(hash_g(g) % (2 ** 31))
    d = dict(x=(4 * r.randint(-4, 5, xs)).astype(np.float32), W=r.randint(-2, 3, ws).astype(np.float32),
             dy=r.randint(-3, 4, ys).astype(np.float32))
    d['prev'] = {k: r.randint(-7, 8, out_shape(k, g)).astype(np.float32) for k in KINDS}
    return d


def real_inputs(g):
    """randn scaled by exp(randn) per sample and channel, as tests/conv_s2_ref.real_inputs draws them"""
    xs, ws, ys = shapes(g)
    r = np.random.RandomState((hash_g(g) + 1000) % (2 ** 31))
    d = dict(x=(r.randn(*xs) * np.exp(r.randn(xs[0], xs[1], 1, 1))).astype(np.float32),
             W=(r.randn(*ws) / np.sqrt(9.0 * ws[1])).astype(np.float32),
             dy=(r.randn(*ys) * np.exp(r.randn(ys[0], ys[1], 1, 1))).astype(np.float32))
    d['prev'] = {k: r.randn(*out_shape(k, g)).astype(np.float32) for k in KINDS}
    return d


def int_magnitude(kind, g):
    """an upper bound of M of the integer inputs, from their ranges: |line| <= 8, |W| <= 2, |dy| <= 3, |previous| <= 7; a
    data-gradient pixel lies on at most two lines, each folded with coefficients of sum 0.5 (1 + 1 + 0.5) over 2 jobs x 3 K"""
    N, C, K, n1, n2 = g
    top = {'fwd': 2 * 3 * C * 2 * 8, 'dgrad': 2 * 1.25 * 6 * K * 2 * 3, 'wgrad': 2 * N * 2 * max(n1, n2) * 3 * 8}[kind]
    return top + 7


# ---- the products as explicit dot products at chosen outputs ----
def _corr9(W):
    """lasagne W [K, C, 3, 3] -> correlation taps [K, C, 9], tap (a, b) at 3 a + b: the packed weights wp[c][tap][k] transposed"""
    return np.ascontiguousarray(np.asarray(W)[:, :, ::-1, ::-1]).reshape(W.shape[0], W.shape[1], 9)


def _rowjob(i, H):
    return np.where(i == 0, 0, np.where(i == H - 2, 1, np.where(i == H - 1, 2, -1)))


def _coljob(j, W):
    return np.where(j == 0, 3, np.where(j == W - 2, 4, np.where(j == W - 1, 5, -1)))


def terms(kind, g, x, W, dy_pp, idx):
    """-> (a, b) of shape [len(idx), n]: out[idx[e]] = sum_t a[e, t] b[e, t], from the line buffers as the kernels form them
    (absent jobs and positions are zero terms), in the dtype of the inputs.  idx [E, 4]: 'fwd' (n, k, i, j) of the FINE output,
    'dgrad' (n, c, m1, m2), 'wgrad' (k, c, a, b) of the lasagne filter"""
    N, C, K, n1, n2 = g
    H, Wd = 2 * n1, 2 * n2
    idx = np.asarray(idx)
    dtype = np.asarray(W).dtype
    w9 = _corr9(W)
    cs, ks = np.arange(C)[None, :], np.arange(K)[None, :]
    A, B = [], []
    if kind == 'fwd':
        FL = lines(x, dtype)
        n, k, i, j = idx.T
        for job, p in ((_rowjob(i, H), j), (_coljob(j, Wd), i)):
            ok, jc = (job >= 0)[:, None], np.maximum(job, 0)
            for t in range(3):
                A.append(np.where(ok, w9[k[:, None], cs, JOB_TAP[jc, t][:, None]], 0))
                B.append(np.where(ok, FL[n[:, None], JOB_LINE[jc][:, None], cs, (p + t)[:, None]], 0))
    elif kind == 'dgrad':
        DYL = dyl(dy_pp, dtype)
        LP = lp_of(n1, n2)
        dt = dtype.type
        n, c, m1, m2 = idx.T
        rowline = np.where(m1 == 0, 0, np.where(m1 == n1 - 1, 1, -1))
        colline = np.where(m2 == 0, 2, np.where(m2 == n2 - 1, 3, -1))
        for line, m, mat in ((rowline, m2, _line_u(np.eye(n2, dtype=dtype), LP)), (colline, m1, _line_u0(np.eye(n1, dtype=dtype), LP))):
            lc = np.maximum(line, 0)
            sign = np.where(lc % 2 == 0, dt(-0.5), dt(0.5))
            for d in range(3):
                ai = 2 * m + d
                cf = np.where(line >= 0, sign * mat[m, ai], dt(0))
                for slot in range(2):
                    job = np.asarray(LINE_JOBS)[lc, slot]
                    ok, jc = ((job >= 0) & (line >= 0))[:, None], np.maximum(job, 0)
                    for t in range(3):
                        A.append(np.where(ok, cf[:, None] * w9[ks, c[:, None], JOB_TAP[jc, t][:, None]], 0))
                        B.append(np.where(ok, DYL[jc[:, None], n[:, None], ks, (ai - t + 2)[:, None]], 0))
    else:
        assert kind == 'wgrad'
        FL, DYL = lines(x, dtype), dyl(dy_pp, dtype)
        k, c, a_, b_ = idx.T
        ta, tb = 2 - a_, 2 - b_                                   # the correlation tap (A, B) of the lasagne entry (a, b)
        P = 2 * max(n1, n2)                                         # (DYL is zero past the shorter line's end)
        pos = np.arange(P)[None, None, :]
        ns = np.arange(N)[None, :, None]
        rowjob, coljob = np.array([0, 2, 1])[ta], np.array([3, 5, 4])[tb]
        for job, sh in ((rowjob, tb), (coljob, ta)):
            A.append(DYL[job[:, None, None], ns, k[:, None, None], 2 + pos].reshape(len(idx), -1))
            B.append(FL[ns, JOB_LINE[job][:, None, None], c[:, None, None], sh[:, None, None] + pos].reshape(len(idx), -1))
    return np.concatenate(A, 1), np.concatenate(B, 1)


def sample_idx(kind, g, count=SAMPLE):
    """output indices for restate32: every border pixel (every tap) of the first and the last (sample, channel) pair, and
    ``count`` random ones"""
    N, C, K, n1, n2 = g
    r = np.random.RandomState((hash_g(g) + 5 + KINDS.index(kind)) % (2 ** 31))
    if kind == 'wgrad':
        taps = np.argwhere(np.ones((3, 3), bool))
        lead = [(0, 0), (K - 1, C - 1)]
        n_lead, pix = (K, C), taps
    else:
        pix = np.argwhere(fine_border(n1, n2) if kind == 'fwd' else border_coarse(g)[0, 0])
        ch = K if kind == 'fwd' else C
        lead = [(0, 0), (N - 1, ch - 1)]
        n_lead = (N, ch)
    grid = np.concatenate([np.concatenate([np.broadcast_to(np.array(l), (len(pix), 2)), pix], 1) for l in lead])
    rnd = np.concatenate([np.stack([r.randint(0, s, count) for s in n_lead], -1), pix[r.randint(0, len(pix), count)]], 1)
    return np.concatenate([grid, rnd])


def at(kind, a, idx):
    """the elements ``idx`` (as ``terms`` takes them) of a result in its own layout (the forward one parity-planar)"""
    idx = np.asarray(idx)
    if kind == 'fwd':
        a = to_hi(np.asarray(a))
    return np.asarray(a)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


def restate32(kind, g, x, W, dy_pp, prev, idx):
    """the product in fp32 numpy at the outputs ``idx``: the rounded line values, every product rounded, ONE sequential fp32
    accumulator over all of them, then the previous value"""
    f = lambda v: np.asarray(v, np.float32)
    a, b = terms(kind, g, f(x), f(W), f(dy_pp), idx)
    acc = np.cumsum(a.astype(np.float32) * b.astype(np.float32), axis=1, dtype=np.float32)[:, -1]
    return (acc + at(kind, f(prev), idx)).astype(np.float32)
