"""Float64 definitions of the fp32 pooling, resampling, loss, update and loss-scale kernels of csrc/elementwise.hip, the
launcher arithmetic that picks a kernel or a grid restated in Python, and the shape tables and input sets of
tests/test_gpu_elementwise_f32.py (shared with tests/test_elementwise_f32_ref.py, which validates the tables, the inputs and
the bounds on the CPU).  numpy only; built on oracle/ops.py wherever the op exists there, and on tests/elementwise_q_ref.py
for the activations, the BatchNorm expressions and the canary helpers.

Per-element bound of every op:  |got - ref| <= k * 2^-24 * M.
  M  float64 magnitude sum of the terms of the element's expression (returned beside the value).  The inputs are exact fp32
     numbers, so a difference or a quotient of two INPUTS carries a relative error of its own size: M is then |ref|.
  k  number of fp32 roundings on the longest path of the kernel's expression plus one, counted from the source (K_* below).
Ops that only move or select values are bit-exact (k = 0).  A ``restate32_*`` function is the kernel's expression in float32
numpy; the CPU module proves that it stays inside k on every input set of the tables.

Through device libm (logf in bce, tanhf behind the instance norm, powf / sqrtf in adam's step size) k cannot be counted:
K_LIBM holds twice the worst figure measured on the MI355X over the tables, rounded up (the figures are in the docstring of
tests/test_gpu_elementwise_f32.py).

Two deliberate differences from Theano ("Tolerances") are the kernels' contract and are encoded here, with inputs
that hit them: the LeakyReLU slope where the OUTPUT is exactly 0 is alpha (Theano: (1 + alpha) / 2), and sign(0) = 0 in the
L1 gradient, so an element with a == b gets gradient exactly 0.

Loss scalars are accumulated in fp64 and rounded once; see K_LOSS.
"""
import numpy as np

from oracle import ops as O
from tests import elementwise_q_ref as Q
from tests.elementwise_q_ref import (U, ALPHA, REL_L2, canary_fill, canary_changed, f32_inside, worst, bits_equal,  # noqa: F401
                                     view_inputs, rel, a32)

ACTS = Q.ACTS
F32MAX = np.float32(3.4028234663852886e38)

# ---- k per op ----
K_EXACT = 0
K_MAXPOOL_BWD = {'linear': 0, 'relu': 0, 'lrelu': 2}   # g * act'(x): the slope is 1 or 0 (exact) or alpha (one product)
K_AVGPOOL_BWD = 2                                       # dy / (p p): one quotient


def k_avgpool_fwd(p):
    """p p - 1 sequential sums, one quotient"""
    return p * p + 1


K_NEAREST_BWD = 3                   # (a.x + a.y) + (b.x + b.y): depth two
K_BILINEAR_FWD = Q.K_BILINEAR
# up_bilinear_bwd_kernel: a row value is at most three sums deep (the halvings are exact), the four row values are summed three
# deep again = 6; up_bilinear_bwd2_kernel: two sums inside a row term, two more over the three rows = 4 (an fma only removes one)
K_BILINEAR_BWD = 7
# scalar_loss_kernel, kind 0: gscale * 2 * e / n with e = v - target: e, the two products, the quotient = 4
K_LSGAN_GRAD = 5
# kind 1: gscale * (-(t / v) + (1 - t) / (1 - v)) / n: 1 - v, the quotients, the sum, the product, the quotient = 6 at most
K_BCE_GRAD = 7
# recon_loss_kernel: w = gscale * g / total with g = 2 (a - b) or its sign: a - b, the product, the quotient = 3
K_RECON_GRAD = 4
# a loss is a float64 sum of per-element terms whose fp32 ingredient e = v - target (a - b) has one rounding -- e * e doubles it
# -- divided in fp64 and rounded once to fp32: 2 + 1/2, against M = the loss itself.  "a few units": 4
K_LOSS = 4
# rmsprop_kernel from its inputs, one launch.  gg = g * gscale (1); acc' = rho * acc + (1 - rho) * gg * gg: 1 - rho, two
# products by gg (each carrying gg's rounding), rho * acc, the sum -> 7 on the larger term; p' = p - lr * gg / sqrtf(acc' + eps):
# the sum and the root (half of acc's 8, + 1), lr * gg (2), the quotient, the difference -> 9
K_RMSPROP_ACC = 8
K_RMSPROP_P = 10
# adam_kernel's m' = b1 m + (1 - b1) gg: 1 - b1, gg, two products, the sum = 5; v' the same with one more product = 6
K_ADAM_M = 6
K_ADAM_V = 7
# instance norm forward: the BatchNorm expression of elementwise_q_ref (K_BN_APPLY) with mean and inv computed by the kernel
# from fp64 sums and rounded to fp32 (one rounding each, against M with |mean| in it) = + 2
K_IN_FWD = {a: k + 2 for a, k in Q.K_BN_APPLY.items() if a != 'tanh'}
K_IN_STATS = 2                      # mean, inv: an fp64 expression rounded once
K_IN_BWD = Q.K_BN_BWD               # from the fp32 mean / inv the forward produced: elementwise_q_ref's count


def k_in_dgamma(instances):
    """dgamma / dbeta: per instance an fp64 sum of fp32 products dz * xhat (dz: 1 rounding, xhat: 2) rounded once (4), then
    summed over the instances and the previous value in fixed order in fp32 (one rounding per instance)"""
    return 5 + instances


# twice the worst |got - ref| / (2^-24 M) measured on the MI355X over the tables below, rounded up
K_LIBM = {
    'bce_loss': 3,          # measured 1.08: an fp64 sum of logf terms, each within an ulp of logf's argument error
    'in_fwd_tanh': 6,       # measured 2.85
    'in_bwd_tanh': 6,       # measured 2.94: act' = 1 - y y with y recomputed by tanhf
    'adam_p': 6,            # measured 2.74: powf, sqrtf in the step size
}


# ---- launcher arithmetic of csrc/elementwise.hip restated ----
def loss_grid(n):
    return int(max(min((n + 2047) // 2048, 1024), 1))


def loss_path(n):
    """'single': the block finishes the loss itself; 'multi': per-block partials + loss_final_kernel; 'capped': the same with
    1024 blocks walking the tensor in a grid-stride loop"""
    g = loss_grid(n)
    return 'single' if g == 1 else ('capped' if g * 2048 < n else 'multi')


def recon_vec(C, HW, a_view, b_view, g_view):
    """ghm_recon_loss's VEC: views are (first element, elements between samples) relative to a 16-byte aligned allocation;
    g_view None: no gradient asked"""
    views = [v for v in (a_view, b_view, g_view) if v is not None]
    return 4 if (C * HW) % 4 == 0 and all(el0 % 4 == 0 and ns % 4 == 0 for el0, ns in views) else 1


def recon_path(N, C, HW, a_view, b_view, g_view):
    return recon_vec(C, HW, a_view, b_view, g_view), loss_path(N * C * HW)


def bilinear_bwd_kernel(N, C, H, W, dx_view):
    """ghm_upsample_bilinear2_bwd -> ('bwd2', blocks per plane) or ('slow', why); dy is a whole allocation"""
    el0, ns = dx_view
    if W % 2:
        return 'slow', 'odd W'
    if ns % 2:
        return 'slow', 'odd dxs'
    if el0 % 2:
        return 'slow', 'dx 4-byte aligned'
    if N * C > 65535:
        return 'slow', 'N C > 65535'
    return 'bwd2', (H * (W // 2) + 255) // 256


def grad_check_grid(n):
    """-> (blocks, float4s of the body, True when the body needs more than one grid sweep, tail elements)"""
    n4c = (n + 3) // 4
    grid = (n4c + 255) // 256 if n4c < 256 * 2048 else 2048
    return grid, n >> 2, (n >> 2) > grid * 256, n & 3


BN_SMALL_MAX = 16384
BN_MAX_SPLIT = 64


def bn_small(count):
    return count <= BN_SMALL_MAX


def bn_split(C, count):
    return int(max(min((1024 + C - 1) // C, max(count // 2048, 1), BN_MAX_SPLIT), 1))


def bn_row_segs(N, C, HW):
    if HW % 4 or N > BN_MAX_SPLIT:
        return 0
    segs = max(min((2048 + C * N - 1) // (C * N), BN_MAX_SPLIT // N, max(HW // 2048, 1)), 1)
    ln = ((HW + segs - 1) // segs + 3) // 4 * 4
    return (HW + ln - 1) // ln


def in_dispatch(group, C, HW, views):
    """ghm_instance_norm_fwd / _bwd call the BatchNorm launchers once per instance with N = group: -> ('small', VEC) for the
    one-launch kernels, ('rows', S, VEC) / ('flat', S, VEC) for the three-pass form (S partials per channel, VEC of the apply
    pass); views: (first element, sample stride) of every tensor of the call"""
    vec = 4 if HW % 4 == 0 and all(el0 % 4 == 0 and ns % 4 == 0 for el0, ns in views) else 1
    if bn_small(group * HW):
        return ('small', vec)
    segs = bn_row_segs(group, C, HW) if vec == 4 else 0
    return ('rows', group * segs, vec) if segs else ('flat', bn_split(C, group * HW), vec)


def view_of(shape, spec):
    """(first element, extra elements between samples) -> (first element, sample stride)"""
    N, C, H, W = shape
    return spec[0], C * H * W + spec[1]


# ---- max-pool 2x2 ----
# (N, C, H, W)
MAXPOOL_ROWS = [
    ((2, 3, 2, 6), "H = 2: one row of windows; 18 windows in one block that spans all six planes"),
    ((2, 3, 6, 2), "W = 2: one window per row pair"),
    ((3, 5, 8, 12), "24 windows per plane, fewer than a block: 360 windows, the second block starts inside plane 10"),
    ((1, 2, 40, 28), "280 windows per plane, more than a block: 560 windows, three blocks"),
]
MAXPOOL_REFUSED = [(1, 2, 3, 4), (1, 2, 4, 5)]


def maxpool_inputs(shape):
    """x on the integer grid -1 .. 1, the larger values more likely (most windows tie; zeros of both signs), plane (0, 0)
    constant; dy normal"""
    N, C, H, W = shape
    r = Q._rng(shape, 11)
    x = r.choice(np.array([-1, 0, 1], np.float32), size=shape, p=[0.2, 0.3, 0.5])
    x[(x == 0) & (r.rand(*shape) < 0.5)] = -0.0
    x[0, 0] = 1.0
    x[-1, -1, :2, :2] = [[0.0, -0.0], [-0.0, -1.0]]            # a window whose maximum is a zero of either sign
    return dict(x=x, dy=r.randn(N, C, H // 2, W // 2).astype(np.float32))


def windows(x):
    N, C, H, W = x.shape
    return x.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def maxpool_fwd(x):
    return O.maxpool_fwd(np.asarray(x, np.float64), 2)


def maxpool_selects(got, x):
    """forward contract of a kernel that only selects: every output equals the window's maximum and carries the bits of one
    of the window's elements (a window of +0.0 and -0.0 may yield either zero)"""
    w = windows(np.ascontiguousarray(x, np.float32))
    g = np.ascontiguousarray(got, np.float32)
    same_bits = (w.view(np.uint32) == g.view(np.uint32)[..., None]).any(-1)
    return bool(np.array_equal(g, w.max(-1)) and same_bits.all())


def maxpool_bwd(x, y, dy, act, alpha=0.0):
    """-> (dx, M): the gradient to EVERY position equal to the maximum, times act'(x) (x is the activation's output)"""
    x64 = np.asarray(x, np.float64)
    dx = O.maxpool_vjp(x64, np.asarray(y, np.float64), np.asarray(dy, np.float64), 2) * Q.dact_from_out(x, act, alpha)
    return dx, np.abs(dx)


def restate32_maxpool_bwd(x, y, dy, act, alpha=0.0):
    x = np.asarray(x, np.float32)
    yu = np.asarray(y, np.float32).repeat(2, 2).repeat(2, 3)
    gu = np.asarray(dy, np.float32).repeat(2, 2).repeat(2, 3)
    return np.where(x == yu, gu * Q.restate32_dact(x, act, alpha), np.float32(0)).astype(np.float32)


# ---- average pool ----
# ((N, C, H, W), p)
AVGPOOL_ROWS = [
    (((2, 3, 8, 12), 2), "p = 2"),
    (((2, 3, 8, 12), 4), "p = 4: the older test's geometry, 576 input elements: three blocks backward"),
    (((1, 2, 16, 8), 8), "p = 8"),
    (((2, 2, 4, 4), 4), "p = H = W: global pooling, one output per plane"),
    (((1, 3, 8, 8), 8), "p = H = W = 8: global pooling"),
    (((2, 3, 7, 9), 2), "H % p = 1, W % p = 1: last row and column ignored forward, zero backward"),
    (((1, 2, 10, 13), 4), "H % p = 2, W % p = 1 with p = 4: two border rows"),
]


def avgpool_fwd(x, p):
    x = np.asarray(x, np.float64)
    return O.avgpool_fwd(x, p), O.avgpool_fwd(np.abs(x), p)


def avgpool_bwd(shape, dy, p):
    dx = O.avgpool_vjp(shape, np.asarray(dy, np.float64), p)
    return dx, np.abs(dx)


def restate32_avgpool_fwd(x, p):
    x = np.asarray(x, np.float32)
    Ho, Wo = x.shape[2] // p, x.shape[3] // p
    s = np.zeros(x.shape[:2] + (Ho, Wo), np.float32)
    for a in range(p):
        for b in range(p):
            s = s + x[:, :, a:Ho * p:p, b:Wo * p:p]
    return (s / np.float32(p * p)).astype(np.float32)


def restate32_avgpool_bwd(shape, dy, p):
    return O.avgpool_vjp(shape, np.asarray(dy, np.float32), p)            # dy / (p p) in float32


# ---- nearest and Theano-bilinear 2x ----
# ((N, C, H, W) of the coarse map, source view, gradient-destination view, large): a view is (first element, extra elements
# between samples) inside a 16-byte aligned allocation; the fine tensors are whole allocations
UP_ROWS = [
    (((2, 3, 1, 1), (0, 0), (0, 0), False), "slow: odd W; 1x1: every index clamped"),
    (((2, 3, 1, 4), (0, 0), (0, 0), False), "bwd2 x 1: H = 1, even W: the only coarse row is first and last"),
    (((2, 3, 5, 7), (0, 0), (0, 0), False), "slow: odd W, odd H"),
    (((2, 3, 4, 2), (0, 0), (0, 0), False), "bwd2 x 1: W = 2: the one column pair is leftmost and rightmost"),
    (((2, 3, 24, 24), (0, 0), (0, 0), False), "bwd2 x 2: H W / 2 = 288 > 256, two blocks per plane"),
    (((2, 3, 6, 4), (24, 48), (24, 48), False), "bwd2 x 1: channel slices 1 .. 3 of five channels, even offset and stride"),
    (((2, 3, 6, 4), (5, 10), (5, 10), False), "slow: dx 4-byte aligned: an odd first element with an even stride"),
    (((2, 3, 6, 4), (24, 7), (24, 7), False), "slow: odd dxs: an even first element with an odd stride"),
    (((21845, 3, 1, 2), (0, 0), (0, 0), True), "bwd2 x 1: N C = 65535 planes in gridDim.y, the most the fast kernel takes"),
    (((21846, 3, 1, 2), (0, 0), (0, 0), True), "slow: N C > 65535 with a tiny even-W map"),
]


def up_inputs(shape):
    N, C, H, W = shape
    r = Q._rng(shape, 12)
    return dict(x=r.randn(*shape).astype(np.float32), g=r.randn(N, C, 2 * H, 2 * W).astype(np.float32),
                prev=r.randn(*shape).astype(np.float32))


def nearest_fwd(x):
    return O.upscale_nearest_fwd(np.asarray(x))


def nearest_bwd(g):
    g = np.asarray(g, np.float64)
    return O.upscale_nearest_vjp(g), O.upscale_nearest_vjp(np.abs(g))


def restate32_nearest_bwd(g):
    g = np.asarray(g, np.float32)
    return (g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + (g[:, :, 1::2, 0::2] + g[:, :, 1::2, 1::2])


def bilinear_fwd(x):
    """-> (Theano's algorithm transcribed, the closed form, M)"""
    x = np.asarray(x, np.float64)
    return O.bilinear_theano_literal(x), O.bilinear_up2_fwd(x), O.bilinear_up2_fwd(np.abs(x))


restate32_bilinear_fwd = Q.restate32_bilinear


def bilinear_bwd(g):
    g = np.asarray(g, np.float64)
    return O.bilinear_up2_vjp(g), O.bilinear_up2_vjp(np.abs(g))


def _restate32_bil_axis(g, axis):
    """bil_row along ``axis``: g[2m] + g[2m+1] / 2, + g[2m-1] / 2 for m >= 1, + g[2n-1] / 2 for m == n - 1, in this order"""
    g = np.moveaxis(np.asarray(g, np.float32), axis, -1)
    h = np.float32(0.5)
    s = g[..., 0::2] + h * g[..., 1::2]
    s[..., 1:] = s[..., 1:] + h * g[..., 1:-2:2]
    s[..., -1] = s[..., -1] + h * g[..., -1]
    return np.moveaxis(s, -1, axis)


def restate32_bilinear_bwd(g):
    out = _restate32_bil_axis(_restate32_bil_axis(g, 3), 2)
    assert out.dtype == np.float32
    return out


# ---- losses ----
LOSS_NS = [
    (1, "single: one element"),
    (2047, "single: the last lane of the eighth sweep is idle"),
    (2048, "single: the largest single-block n"),
    (2049, "multi: two blocks taking runs of 256 elements in turn, the last run one element long"),
    (16384, "multi: a PatchGAN-sized map, eight blocks"),
    (2 ** 21 + 5, "capped: 1025 blocks wanted, 1024 launched, grid-stride loop"),
]


def loss_inputs(n, kind):
    r = np.random.RandomState(n % 9973 + (7 if kind == 'bce' else 0))
    d = (r.rand(n) * 0.8 + 0.1).astype(np.float32) if kind == 'bce' else r.randn(n).astype(np.float32)
    return d.reshape(n, 1, 1, 1)


def scalar_loss(d, target, kind, gscale):
    """-> (loss, M of the loss, grad, M of the grad)"""
    d = np.asarray(d, np.float64)
    if kind == 'lsgan':
        loss, g = O.squared_error_mean(d, target)
        return loss, abs(loss), gscale * g, np.abs(gscale * g)
    t = float(target)
    loss, g = O.bce_mean(d, t)
    return loss, np.abs(t * np.log(d)).mean() + np.abs((1 - t) * np.log(1 - d)).mean(), gscale * g, np.abs(gscale * g)


def restate32_scalar_loss(d, target, kind, gscale):
    d = np.asarray(d, np.float32)
    n, t, gs, one = np.float32(d.size), np.float32(target), np.float32(gscale), np.float32(1)
    if kind == 'lsgan':
        e = d - t
        loss = np.float32((e.astype(np.float64) ** 2).sum() / d.size)
        return loss, (gs * np.float32(2) * e / n).astype(np.float32)
    lg = lambda v: np.log(v.astype(np.float64)).astype(np.float32)          # logf taken as correctly rounded
    term = -(t * lg(d) + (one - t) * lg(one - d))
    loss = np.float32(term.astype(np.float64).sum() / d.size)
    return loss, (gs * (-(t / d) + (one - t) / (one - d)) / n).astype(np.float32)


# ((N, C, H, W), l2, view of a, of b, of the gradient, grad_scale)
RECON_ROWS = [
    (((2, 3, 16, 16), False, (0, 0), (0, 0), (0, 0), 100.0), "VEC 4, single: the older test's geometry, L1"),
    (((2, 3, 16, 16), True, (0, 0), (0, 0), (0, 0), 0.5), "VEC 4, single: L2"),
    (((2, 3, 5, 7), False, (0, 0), (0, 0), (0, 0), 100.0), "VEC 1, single: C HW = 105"),
    (((2, 3, 5, 7), True, (3, 5), (0, 0), (7, 11), 0.5), "VEC 1, single: three different odd strides"),
    (((2, 4, 8, 8), False, (0, 0), (64, 128), (32, 64), 100.0), "VEC 4, single: three different strides, all multiples of four"),
    (((2, 4, 8, 8), True, (0, 0), (2, 4), (0, 0), 0.5), "VEC 1, single: C HW % 4 == 0 but b starts 8 bytes into a unit"),
    (((2, 3, 40, 40), False, (0, 0), (1600, 3200), (0, 0), 100.0), "VEC 4, multi: five blocks"),
    (((2, 3, 41, 39), True, (0, 0), (0, 0), (0, 0), 0.5), "VEC 1, multi: C HW = 4797"),
    (((2, 3, 592, 592), False, (0, 0), (0, 0), (0, 0), 100.0), "VEC 4, capped: 2102784 elements, the grid-stride loop"),
]


def recon_inputs(shape):
    """a, b with one element in eight equal (sign(0) = 0, and a zero L2 gradient), and a previous gradient"""
    r = Q._rng(shape, 13)
    a, b = r.randn(*shape).astype(np.float32), r.randn(*shape).astype(np.float32)
    eq = r.rand(*shape) < 0.125
    b[eq] = a[eq]
    return dict(a=a, b=b, prev=r.randn(*shape).astype(np.float32))


def recon_loss(a, b, l2, gscale):
    """-> (loss, grad, M of the grad); M of the loss is the loss"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    loss, g = (O.l2_mean if l2 else O.l1_mean)(a, b)
    return loss, gscale * g, np.abs(gscale * g)


def restate32_recon_loss(a, b, l2, gscale):
    dlt = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    tot, gs = np.float32(dlt.size), np.float32(gscale)
    if l2:
        return np.float32((dlt.astype(np.float64) ** 2).sum() / dlt.size), (gs * (np.float32(2) * dlt) / tot).astype(np.float32)
    return np.float32(np.abs(dlt).astype(np.float64).sum() / dlt.size), (gs * np.sign(dlt) / tot).astype(np.float32)


# ---- rmsprop / adam, one launch from given states (the five-launch protocol is in tests/test_gpu_optimizers.py) ----
OPT_NS = [(1003, "tail of three after 250 float4"), (4096, "no tail"), (5, "one float4 and a tail of one")]
RMSPROP_CONSTS = (0.85, 1e-5)       # rho, eps: not the defaults, so a swapped or dropped constant shows
ADAM_CONSTS = (0.8, 0.99, 1e-7)     # b1, b2, eps
ADAM_T0 = (0.0, 1e5)


def opt_inputs(n):
    r = np.random.RandomState(n)
    return dict(p=(r.randn(n) * 0.1).astype(np.float32), g=r.randn(n).astype(np.float32), acc=np.abs(r.randn(n)).astype(np.float32),
                m=(r.randn(n) * 0.3).astype(np.float32))


def f64(*xs):
    """the constants as the kernel receives them: fp32 values"""
    return tuple(float(np.float32(x)) for x in xs)


def rmsprop(p, g, acc, lr, rho, eps, gscale):
    """-> (p', M, acc', M) of oracle.ops.rmsprop_step on gscale * g"""
    p, g, acc = (np.asarray(v, np.float64) for v in (p, g, acc))
    lr, rho, eps, gscale = f64(lr, rho, eps, gscale)
    gg = g * gscale
    p2, a2 = O.rmsprop_step(p, gg, acc, lr, rho, eps)
    return p2, np.abs(p) + np.abs(p2 - p), a2, a2


def restate32_rmsprop(p, g, acc, lr, rho, eps, gscale):
    f = np.float32
    p, g, acc = (np.asarray(v, f) for v in (p, g, acc))
    gg = g * f(gscale)
    a2 = f(rho) * acc + (f(1) - f(rho)) * gg * gg
    return (p - f(lr) * gg / np.sqrt(a2 + f(eps))).astype(f), a2.astype(f)


def adam(p, g, m, v, t_prev, lr, b1, b2, eps, gscale):
    """-> (p', M, m', M, v', M) of oracle.ops.adam_step on gscale * g"""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, gscale = f64(lr, b1, b2, eps, gscale)
    gg = g * gscale
    p2, m2, v2, _ = O.adam_step(p, gg, m, v, float(t_prev), lr, b1, b2, eps)
    return p2, np.abs(p) + np.abs(p2 - p), m2, np.abs(b1 * m) + np.abs((1 - b1) * gg), v2, v2


def restate32_adam(p, g, m, v, t_prev, lr, b1, b2, eps, gscale):
    f = np.float32
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    t = f(t_prev) + f(1)
    pw = lambda b: f(np.float64(f(b)) ** np.float64(t))                     # powf taken as correctly rounded
    a_t = f(lr) * np.sqrt(f(1) - pw(b2)) / (f(1) - pw(b1))
    gg = g * f(gscale)
    m2 = f(b1) * m + (f(1) - f(b1)) * gg
    v2 = f(b2) * v + (f(1) - f(b2)) * gg * gg
    return (p - a_t * m2 / (np.sqrt(v2) + f(eps))).astype(f), m2.astype(f), v2.astype(f)


# ---- overflow check and the loss-scale state {scale, 1 / scale, good steps, overflow flag, skipped steps, -, -, -} ----
GRAD_CHECK_NS = [
    (1, "1 block, no float4, a tail of one"),
    (3, "1 block, no float4, a tail of three"),
    (4, "1 block, one float4, no tail"),
    (5, "1 block, one float4, a tail of one"),
    (1023, "1 block, 255 float4, a tail of three"),
    (2 ** 21 + 7, "2048 blocks, a second grid sweep of one float4, a tail of three"),
]
NONFINITE = [0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7f800001]       # +Inf, -Inf, a quiet NaN, NaNs with payloads
FINITE_EXTREMES = [0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x80000000, 0x00800000]


def grad_check_positions(n):
    """indices at which one non-finite value is planted: 0, both ends of the last full float4, every tail position and -- past
    one grid sweep -- the last element of the first sweep and the first of the second"""
    grid, n4, swept, tail = grad_check_grid(n)
    pos = {0}
    if n4:
        pos |= {4 * n4 - 4, 4 * n4 - 1}
    pos |= {4 * n4 + t for t in range(tail)}
    if swept:
        pos |= {4 * grid * 256 - 1, 4 * grid * 256}
    return sorted(pos)


def loss_scale_update(ls, interval, lo, hi):
    """loss_scale_update_kernel on a float32 state vector, restated"""
    f = np.float32
    ls = np.array(ls, f)
    s, good = ls[0], ls[2]
    if ls[3] != 0:
        s, good = max(s * f(0.5), f(lo)), f(0)
        ls[4] += f(1)
    else:
        good = good + f(1)
        if good >= f(interval):
            s, good = min(s * f(2), f(hi)), f(0)
    ls[0], ls[1], ls[2], ls[3] = s, f(1) / s, good, 0
    return ls


# (interval, lo, hi, first scale, 1 = the step overflows)
LOSS_SCALE_RUNS = [
    (3, 1.5, 5.0, 4.0, [1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0]),
    (2000, 1.0, 2.0 ** 24, 2.0 ** 15, [0, 1, 0, 0, 1, 1]),          # the defaults: no doubling in six steps
]


# ---- instance norm ----
# ((N, C, H, W), group, act, view of x, of y and dx, accumulate dgamma / dbeta)
IN_ROWS = [
    (((4, 3, 16, 16), 1, 'lrelu', (0, 0), (0, 0), False), "small 4: HW = 256, four instances"),
    (((4, 3, 16, 16), 2, 'relu', (0, 0), (0, 0), True), "small 4: group 2, two instances of 512 values per channel"),
    (((4, 64, 16, 16), 2, 'linear', (256, 512), (256, 512), False), "small 4: C = 64, channel slices of 66 channels"),
    (((2, 3, 16, 16), 1, 'tanh', (0, 0), (0, 0), True), "small 4: tanh"),
    (((2, 3, 15, 17), 1, 'lrelu', (255, 510), (0, 0), True), "small 1: HW = 255, x a channel slice (odd stride)"),
    (((2, 3, 128, 128), 1, 'lrelu', (0, 0), (0, 0), False), "small 4: HW = 16384, the last one-launch size"),
    (((1, 3, 127, 129), 1, 'relu', (0, 0), (0, 0), False), "small 1: HW = 16383, odd, below the threshold"),
    (((2, 3, 4097, 4), 1, 'lrelu', (0, 0), (16388, 32776), True), "rows: HW = 16388, S = 8, VEC 4; y / dx channel slices"),
    (((1, 3, 5, 3277), 1, 'linear', (0, 0), (0, 0), False), "flat: HW = 16385, odd, above the threshold: S = 8, VEC 1"),
    (((2, 3, 256, 256), 1, 'tanh', (0, 0), (0, 0), False), "rows: HW = 65536, S = 32, VEC 4"),
    (((4, 3, 128, 128), 2, 'relu', (0, 0), (0, 0), True), "rows: group 2 of HW = 16384: 32768 values per channel, S = 16, VEC 4"),
    (((1, 64, 4097, 4), 1, 'lrelu', (0, 0), (0, 0), False), "rows: C = 64, S = 8, VEC 4"),
]
IN_REFUSED = ((3, 3, 4, 4), 2)
IN_EPS = 1e-4


def in_inputs(shape, group=1):
    """x with per-(sample, channel) offsets and spreads and one constant instance plane (var = 0); dout with a mean and a component
    along x; gamma, beta; previous dgamma / dbeta"""
    N, C, H, W = shape
    r = Q._rng(shape, 14)
    x = (r.randn(*shape) * (0.5 + 2 * r.rand(N, C, 1, 1)) + r.randn(N, C, 1, 1)).astype(np.float32)
    x[:group, C - 1] = 0.75
    dout = (r.randn(*shape) + 0.5 + 0.3 * x).astype(np.float32)
    return dict(x=x, dout=dout, gamma=(r.rand(C) + 0.5).astype(np.float32), beta=r.randn(C).astype(np.float32),
                prev=r.randn(2, C).astype(np.float32))


def to_groups(x, group):
    """[N, C, H, W] -> [N / group, C, group H, W]: ``group`` consecutive samples are ONE instance, whose statistics run over the
    maps of all its samples"""
    N, C, H, W = x.shape
    return np.ascontiguousarray(x.reshape(N // group, group, C, H, W).transpose(0, 2, 1, 3, 4)).reshape(N // group, C, group * H, W)


def from_groups(xg, group):
    I, C, GH, W = xg.shape
    H = GH // group
    return np.ascontiguousarray(xg.reshape(I, C, group, H, W).transpose(0, 2, 1, 3, 4)).reshape(I * group, C, H, W)


def instance_norm_fwd(x, gamma, beta, act, alpha=0.0, group=1, eps=IN_EPS):
    """oracle.ops.in_fwd over the groups, the activation behind it -> (y, M, mean [N / group, C], inv)"""
    xg = to_groups(np.asarray(x, np.float64), group)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    pre, mu, inv = O.in_fwd(xg, beta, gamma, float(np.float32(eps)))
    sc = np.abs(gamma[None, :] * inv)[:, :, None, None]
    M = (np.abs(xg) + np.abs(mu)[:, :, None, None]) * sc + np.abs(beta)[None, :, None, None]
    return from_groups(Q.act_fwd(pre, act, alpha), group), from_groups(M, group), mu, inv


def instance_norm_bwd(dout, y, x, mean, inv, gamma, act, alpha=0.0, group=1):
    """from the fp32 statistics and output of the forward -> (dx, M, dgamma, M, dbeta, M): elementwise_q_ref.bn_backward per
    instance (== oracle.ops.in_vjp behind the activation's derivative), the parameter gradients summed over the instances"""
    dg_, yg, xg = (to_groups(np.asarray(v), group) for v in (dout, y, x))
    dx, M = np.empty(xg.shape), np.empty(xg.shape)
    C = xg.shape[1]
    dg, db, Mg, Mb = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    for i in range(xg.shape[0]):
        sl = slice(i, i + 1)
        dx[sl], M[sl], a, b = Q.bn_backward(dg_[sl], yg[sl], xg[sl], mean[i], inv[i], gamma, act, alpha)
        dz = dg_[sl].astype(np.float64) * Q.dact_from_out(yg[sl], act, alpha)
        xh = (xg[sl].astype(np.float64) - Q._sh(mean[i])) * Q._sh(inv[i])
        if act == 'tanh':           # act' = 1 - y y: the magnitude sum of its terms is 1 + y y, not |1 - y y|
            M[sl] += np.abs(Q._sh(gamma) * Q._sh(inv[i]) * dg_[sl]) * 2 * yg[sl].astype(np.float64) ** 2
        dg, db = dg + a, db + b
        adz = np.abs(dg_[sl]) * (1 + yg[sl].astype(np.float64) ** 2) if act == 'tanh' else np.abs(dz)
        Mg, Mb = Mg + (adz * np.abs(xh)).sum(axis=(0, 2, 3)), Mb + adz.sum(axis=(0, 2, 3))
    return from_groups(dx, group), from_groups(M, group), dg, Mg, db, Mb


def restate32_instance_norm_fwd(x, gamma, beta, act, alpha=0.0, group=1, eps=IN_EPS):
    """statistics from fp64 sums rounded once, then elementwise_q_ref.restate32_bn_apply per instance"""
    xg = to_groups(np.asarray(x, np.float32), group)
    out = np.empty(xg.shape, np.float32)
    for i in range(xg.shape[0]):
        v = xg[i].astype(np.float64)
        mu = v.mean(axis=(1, 2))
        var = np.maximum((v * v).mean(axis=(1, 2)) - mu * mu, 0)
        inv = (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32)
        out[i] = Q.restate32_bn_apply(xg[i:i + 1], mu.astype(np.float32), inv, gamma, beta, act, alpha)[0]
    return from_groups(out, group)


# ---- axpby ----
def axpby_b0(a, x):
    """b == 0: y = a x + 0, y's previous contents not read"""
    return (np.float32(a) * np.asarray(x, np.float32) + np.float32(0)).astype(np.float32)
