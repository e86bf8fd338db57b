"""Float64 definitions of the fp32 BatchNorm entry points of csrc/elementwise.hip (ghm_bn_stats / _apply / _forward / _backward /
_backward_x), of ghm_channel_sum (csrc/conv_igemm.hip), ghm_scale_samples and the fp32 <-> bf16 kernels behind
ghm_allreduce_sum_bf16 (csrc/comm.hip); their launcher arithmetic restated in Python; and the row tables and input sets of
tests/test_gpu_bn_f32.py (shared with tests/test_bn_f32_ref.py, which validates the tables, the inputs and the bounds on the CPU).
numpy only; built on oracle/lp.py and on the two predecessors (tests/test_bn_f32_ref.py holds the definitions here to
oracle/ops.py): tests/elementwise_f32_ref.py (bn_small, bn_split,
bn_row_segs, the K_IN_* counts) and tests/elementwise_q_ref.py (bn_apply, bn_backward, their fp32 restatements and counts).

Per-element (per-channel) bound of every op:  |got - ref| <= k * 2^-24 * M, k counted from the source, M the float64 magnitude
sum of the terms -- the convention of the two predecessors.  The only figures taken from measurement are K_LIBM's tanh entries.
"""
import numpy as np

from oracle import lp as LP
from tests import elementwise_q_ref as Q
from tests.elementwise_f32_ref import (U, ALPHA, REL_L2, worst, rel, bits_equal, bn_small, bn_split, bn_row_segs,  # noqa: F401
                                       BN_MAX_SPLIT, BN_SMALL_MAX, K_IN_STATS, K_IN_FWD, K_IN_BWD, K_LIBM, k_in_dgamma, view_of)

EPS = 1e-4
RUN_ALPHA = 0.1
# bn_fwd_small_kernel / bn_stats_final: run = (1.f - ra) * run + ra * m: the difference, two products, the sum = 4 roundings (a
# contraction into an fma only removes one), + 1; M = |(1 - ra) run| + |ra m|, m the fp32 value the kernel stored
K_RUN = 5
# dz = dout * act'(y) has one rounding for the piecewise-linear activations (k_in_dgamma's count); tanh's act' = 1 - y y adds the
# product and the difference, against a magnitude sum with 1 + y y in it
K_DGAMMA_TANH_EXTRA = 2
# ghm_scale_samples: (float)((double)x * ((double)num / (double)den)): the fp64 ratio's rounding is 2^-29 units, the result is
# rounded once = 1 rounding + 1
K_SCALE = 2


def k_dgamma(act):
    return k_in_dgamma(1) + (K_DGAMMA_TANH_EXTRA if act == 'tanh' else 0)


# ---- launcher arithmetic of ghm_bn_stats / _apply / _forward / bn_backward_impl restated ----
def _al(view):
    """a view (first element, sample stride) inside a 16-byte aligned allocation allows 16-byte loads"""
    return view[0] % 4 == 0 and view[1] % 4 == 0


def bn_sum_form(N, C, HW, views, no_small=False):
    """the reduction of a BatchNorm pass over tensors at ``views`` -> ('small', 1, VEC) | ('rows', S, 4) | ('flat', S, 1 | 4):
    S partials per channel in the workspace, VEC of the loads of the reduction"""
    vec = 4 if HW % 4 == 0 and all(_al(v) for v in views) else 1
    if bn_small(N * HW) and not no_small:
        return 'small', 1, vec
    segs = bn_row_segs(N, C, HW) if vec == 4 else 0
    return ('rows', N * segs, 4) if segs else ('flat', bn_split(C, N * HW), vec)


def bn_dispatch(shape, vx, vy, vd, no_small=False):
    """-> dict: 'stats' (ghm_bn_stats: x alone), 'fwd' (ghm_bn_forward: the same reduction; the VEC of its apply pass from x and
    y), 'bwd' (bn_backward_impl: the reduction from dout, y, x; the VEC of its apply pass with dx, which shares y's view)"""
    N, C, H, W = shape
    x, y, d = view_of(shape, vx), view_of(shape, vy), view_of(shape, vd)
    stats = bn_sum_form(N, C, H * W, [x], no_small)
    app = 4 if (H * W) % 4 == 0 and _al(x) and _al(y) else 1
    fwd = ('small', 1, app) if stats[0] == 'small' else stats[:2] + (app,)
    return dict(stats=stats, fwd=fwd, bwd=bn_sum_form(N, C, H * W, [d, y, x], no_small))


def seg_len(N, C, HW):
    segs = max(min((2048 + C * N - 1) // (C * N), BN_MAX_SPLIT // N, max(HW // 2048, 1)), 1)
    return ((HW + segs - 1) // segs + 3) // 4 * 4


def bn_sum_chain(form, N, C, HW):
    """longest chain of fp64 additions from an element to the per-channel sum: the thread's sequential adds (+ 2 for the tree
    inside a float4), six shuffle steps, three LDS adds, S partials"""
    kind, S, vec = form
    if kind == 'small':
        it = -(-(N * HW // vec) // 256)
    elif kind == 'rows':
        it = -(-seg_len(N, C, HW) // 1024)
    else:
        it = -(-(-(-N * HW // S)) // 256)
    return it + (2 if vec == 4 else 0) + 6 + 3 + (S if kind != 'small' else 0)


def inv_conditioning(mu, var, L, eps=EPS):
    """relative error of inv = 1 / sqrt(E[x^2] - mu^2 + eps) evaluated in fp64 (u = 2^-53) from sums whose longest chain has L
    additions.  The squares of fp32 values are exact in fp64.  sum x: |error| <= L u sum|x|, so mu^2 is off by at most
    (2 L + 3) u |mu| E|x| <= (2 L + 3) u E[x^2]; E[x^2] by (L + 1) u E[x^2]; the difference rounds once more:
    |error of var| <= (3 L + 5) u E[x^2].  inv moves by half of that over var + eps; the sum with eps, the root and the quotient
    add 3 u.  A channel of ONE value (N HW = 1) has none of this: x^2 and mu^2 are the same fp64 number and var is exactly 0."""
    ex2 = np.asarray(mu, np.float64) ** 2 + var
    return ((3 * L + 5) / 2 * ex2 / (np.asarray(var, np.float64) + float(np.float32(eps))) + 3) * 2.0 ** -53


def inv_M(shape, mu, var, inv, L):
    """M of inv: inv itself, widened by the conditioning term in units of 2^-24 (not for a channel of one value)"""
    one = shape[0] * shape[2] * shape[3] == 1
    return inv * (1 + (3 * 2.0 ** -53 if one else inv_conditioning(mu, var, L)) / U)


# ---- BatchNorm rows ----
# ((N, C, H, W), view of x, view of y and dx [, view of dout], activations): a view is (first element, extra elements between
# samples) inside a 16-byte aligned allocation; one view for y / dx / dout, or (view of y and dx, view of dout).
# The note names the reduction ("small V" with the VEC of the one-launch kernels; "rows" / "flat" with S and the VEC of the apply
# passes), checked by tests/test_bn_f32_ref.py.  NO_SMALL rows run under GHM_NO_BN_SMALL=1.
A3 = ('linear', 'relu', 'lrelu')
A4 = A3 + ('tanh',)
BN_ROWS = [
    (((8, 3, 4, 4), (0, 0), (0, 0), A4), "small 4: eight samples of four float4 units, the loop crosses samples inside one pass; tanh"),
    (((64, 2, 16, 16), (0, 0), (0, 0), A3), "small 4: 16384 values per channel, the last one-launch size, with N = 64"),
    (((5, 3, 3, 5), (0, 0), (0, 0), A3), "small 1: HW = 15"),
    (((6, 4, 4, 4), (3, 5), (0, 0), A3), "small 1: HW % 4 == 0 but x starts at an odd element with an odd stride"),
    (((1, 4, 1, 1), (0, 0), (0, 0), A3), "small 1: N HW = 1: variance 0, y = act(beta), dx pure cancellation"),
    (((4, 24, 1, 1), (0, 0), (0, 0), A3), "small 1: 1x1 maps, four samples"),
    (((3, 2, 43, 127), (0, 0), (0, 0), A3), "small 1: 16383 values per channel, odd HW, one below the threshold"),
    (((64, 2, 65, 4), (0, 0), (0, 0), A3), "rows: S = 64, VEC 4: count 16640, segs = 1, S = N = BN_MAX_SPLIT: the last workspace slot of a channel"),
    (((5, 1, 1025, 4), (0, 0), (0, 0), A4), "rows: S = 10, VEC 4: HW = 4100, segs = 2, seg_len 2052, a ragged last segment of 2048; tanh"),
    (((65, 2, 16, 16), (0, 0), (0, 0), A3), "flat: S = 8, VEC 4: N > 64, count 16640, chunks of 2080 straddle samples"),
    (((3, 2, 43, 129), (0, 0), (0, 0), A3), "flat: S = 8, VEC 1: odd HW = 5547, count 16641 above the threshold"),
    (((1, 1, 1, 131073), (0, 0), (0, 0), A3), "flat: S = 64, VEC 1: bn_split reaches BN_MAX_SPLIT"),
    (((2, 257, 2, 2), (0, 0), (0, 0), A3), "rows: S = 2, VEC 4: GHM_NO_BN_SMALL, two blocks of bn_stats_final / bn_bwd_final, the second one thread"),
    (((4, 3, 4, 4), (16, 32), ((32, 64), (0, 16)), A3), "small 4: channel slices of 5, 7 and 4 channels: strides 80, 112, 64"),
    (((2, 3, 2049, 4), (8196, 16392), ((0, 8196), (16392, 24588)), A3), "rows: S = 8, VEC 4: channel slices of 5, 4 and 6 channels, HW = 8196"),
]
NO_SMALL = {(2, 257, 2, 2)}


def row_views(row):
    """-> (shape, view of x, view of y and dx, view of dout, activations)"""
    shape, vx, vy, acts = row
    vy, vd = vy if isinstance(vy[0], tuple) else (vy, vy)
    return shape, vx, vy, vd, acts


ROLES = ('mean1000', 'constant', 'large', 'ordinary')
MEAN, SPREAD = 1000.0, 0.5      # spread 0.01 (ratio E[x^2] / (var + eps) = 5e9) puts the fp64 conditioning term at ~600 ulp of inv
CONST = 0.75


def variants(C):
    """input sets per row: enough rotations of the four channel roles that every role occurs"""
    return 1 if C >= 4 else -(-4 // C)


def role(c, v=0, C=4):
    """the role of channel c of a C-channel tensor in input set v"""
    return ROLES[(c + v * C) % 4]


def bn_inputs(shape, v=0):
    """elementwise_q_ref.bn_inputs extended.  Channel c plays role(c, v): mean 1000 with spread 0.5 (fp32 sums lose its
    variance); constant 0.75 with beta = 0 (variance 0, and a pre-activation of exactly 0: the slope of relu / lrelu AT 0);
    +-large values up to 1e18 (x^2 finite in fp64, every result finite in fp32); ordinary ones with their own offsets and
    spreads.  dout has a mean and a component along x; running statistics and previous dgamma / dbeta are random."""
    N, C, H, W = shape
    d = Q.bn_inputs(shape)
    r = Q._rng(shape, 21 + v)
    x, beta = d['x'].copy(), d['beta'].copy()
    for c in range(C):
        k = role(c, v, C)
        if k == 'mean1000':
            e = r.randn(N, H, W)
            if e.size > 1:
                e = (e - e.mean()) / e.std()                        # the spread is SPREAD whatever the count
            x[:, c] = (MEAN + SPREAD * e).astype(np.float32)
        elif k == 'constant':
            x[:, c], beta[c] = CONST, 0.0
        elif k == 'large':
            x[:, c] = (1e18 * (2 * r.rand(N, H, W) - 1)).astype(np.float32)
    mu, _, inv = bn_stats(x)
    xh = (x.astype(np.float64) - mu.reshape(1, C, 1, 1)) * inv.reshape(1, C, 1, 1)
    dout = (r.randn(*shape) + 0.5 + 0.3 * xh).astype(np.float32)
    return dict(x=x, gamma=d['gamma'], beta=beta, dout=dout, run=np.stack([r.randn(C), r.rand(C) + 0.5]).astype(np.float32),
                prev=r.randn(2, C).astype(np.float32))


def bn_stats(x, eps=EPS):
    """two-pass float64 statistics -> (mu, var, inv)"""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=(0, 2, 3))
    var = ((x - mu.reshape(1, -1, 1, 1)) ** 2).mean(axis=(0, 2, 3))
    return mu, var, 1.0 / np.sqrt(var + float(np.float32(eps)))


def bn_forward(x, gamma, beta, act, alpha=0.0, eps=EPS):
    """oracle.ops.bn_train_fwd's expression from the two-pass statistics, the activation behind it -> (y, M, mu, var, inv); M has
    |mu| in it: the kernel rounds the mean to fp32 before it subtracts"""
    x = np.asarray(x, np.float64)
    mu, var, inv = bn_stats(x, eps)
    sc = Q._sh(gamma) * Q._sh(inv)
    y = Q.act_fwd((x - Q._sh(mu)) * sc + Q._sh(beta), act, alpha)
    return y, (np.abs(x) + np.abs(Q._sh(mu))) * np.abs(sc) + np.abs(Q._sh(beta)), mu, var, inv


def bn_backward(dout, y, x, mean, inv, gamma, act, alpha=0.0):
    """elementwise_q_ref.bn_backward from the fp32 statistics and output of the forward -> (dx, M, dgamma, M, dbeta, M)"""
    dx, M, dg, db = Q.bn_backward(dout, y, x, mean, inv, gamma, act, alpha)
    dz = np.asarray(dout, np.float64) * Q.dact_from_out(y, act, alpha)
    xh = (np.asarray(x, np.float64) - Q._sh(mean)) * Q._sh(inv)
    adz = np.abs(dz)
    if act == 'tanh':               # act' = 1 - y y: the magnitude sum of its terms is 1 + y y
        y2 = np.asarray(y, np.float64) ** 2
        M = M + np.abs(Q._sh(gamma) * Q._sh(inv) * dout) * 2 * y2
        adz = np.abs(dout) * (1 + y2)
    return dx, M, dg, (adz * np.abs(xh)).sum(axis=(0, 2, 3)), db, adz.sum(axis=(0, 2, 3))


def running(run, stat32, ra=RUN_ALPHA):
    """(1 - ra) run + ra stat in float64 of the fp32 values the kernel was given and stored -> (value, M)"""
    ra = float(np.float32(ra))
    a, b = (1 - ra) * np.asarray(run, np.float64), ra * np.asarray(stat32, np.float64)
    return a + b, np.abs(a) + np.abs(b)


def restate32_bn_stats(x, eps=EPS, sums=np.float64):
    """mean and inv of the kernels: one-pass sums in ``sums`` precision (fp64 in the kernels), E[x^2] - mu^2 clamped at 0, both
    rounded once"""
    x = np.asarray(x, np.float32)
    n = x.size // x.shape[1]
    a = x.sum(axis=(0, 2, 3), dtype=sums).astype(np.float64)
    b = (x.astype(sums) * x.astype(sums)).sum(axis=(0, 2, 3), dtype=sums).astype(np.float64)
    mu = a / n
    var = np.maximum(b / n - mu * mu, 0.0)
    return mu.astype(np.float32), (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32)


def restate32_running(run, stat32, ra=RUN_ALPHA):
    f = np.float32
    return ((f(1) - f(ra)) * np.asarray(run, f) + f(ra) * np.asarray(stat32, f)).astype(f)


def restate32_bn_backward(dout, y, x, mean, inv, gamma, act, alpha=0.0, sums=None):
    """elementwise_q_ref.restate32_bn_backward with the two per-channel sums returned, or taken from ``sums``
    -> (dx, sum dz, sum dz xhat)"""
    s = lambda v: np.asarray(v, np.float32).reshape(1, -1, 1, 1)
    dz = (np.asarray(dout, np.float32) * Q.restate32_dact(y, act, alpha)).astype(np.float32)
    xh = ((np.asarray(x, np.float32) - s(mean)) * s(inv)).astype(np.float32)
    if sums is None:
        sums = (dz.astype(np.float64).sum(axis=(0, 2, 3)).astype(np.float32), (dz.astype(np.float64) * xh).sum(axis=(0, 2, 3)).astype(np.float32))
    ic = np.float32(1) / np.float32(dz.size // dz.shape[1])
    g, mb, mg = s(gamma) * s(inv), s(sums[0] * ic), s(sums[1] * ic)
    return (g * ((dz - mb) - xh * mg)).astype(np.float32), sums[0], sums[1]


# ---- ghm_channel_sum ----
def cs_dispatch(shape, spec):
    """-> (S, chunk, 'vector' | 'scalar'): S = min(ceil(1024 / C), max(total / 4096, 1), 256) blocks per channel over runs of
    ``chunk`` elements (rounded up to 4); the float4 loop needs HW % 4 == 0, nstride % 4 == 0 and a 16-byte aligned pointer"""
    N, C, H, W = shape
    total = N * H * W
    S = min((1024 + C - 1) // C, max(total // 4096, 1), 256)
    chunk = ((total + S - 1) // S + 3) & ~3
    el0, ns = view_of(shape, spec)
    return S, chunk, 'vector' if (H * W) % 4 == 0 and ns % 4 == 0 and el0 % 4 == 0 else 'scalar'


def k_channel_sum(shape, spec, accumulate):
    """longest chain of fp32 additions to the result, + 1: the thread's sequential adds (vector: one per sweep of 4096 elements,
    the float4 tree and the s4 tree, two each), six shuffle steps, the LDS tree (2), S partials, one for ``accumulate``"""
    S, chunk, path = cs_dispatch(shape, spec)
    it = -(-chunk // 4096) + 4 if path == 'vector' else -(-chunk // 256)
    return it + 6 + 2 + (S if S > 1 else 0) + (1 if accumulate else 0) + 1


# ((N, C, H, W), view of x)
CS_ROWS = [
    (((2, 5, 7, 9), (0, 0)), "S = 1, scalar: direct write"),
    (((2, 3, 64, 64), (0, 0)), "S = 2, vector"),
    (((3, 2, 64, 65), (0, 0)), "S = 3, vector: HW = 4160, a block per sample"),
    (((3, 2, 63, 65), (0, 0)), "S = 2, scalar: total 12285, the chunk 6143 rounded up to 6144, the last one 6141 long, chunks straddle samples"),
    (((1, 1, 1024, 1024), (0, 0)), "S = 256, vector: the cap"),
    (((1, 300, 64, 64), (0, 0)), "S = 1, vector: C > 256 in gridDim.y, direct write (no final kernel)"),
    (((2, 257, 64, 64), (0, 0)), "S = 2, vector: C > 256 with partials: two blocks of channel_sum_final, the second one thread"),
    (((1, 2, 3, 4100), (0, 0)), "S = 3, vector: chunk 4100 is no multiple of the 4096-element sweep: the ek < hi guards decide"),
    (((2, 3, 64, 64), (4096, 8192)), "S = 2, vector: a channel slice of five channels, nstride != C HW"),
    (((2, 3, 64, 64), (1, 0)), "S = 2, scalar: HW % 4 == 0 and nstride % 4 == 0 but the view starts at an odd element"),
    (((2, 4, 4, 4), (3, 0)), "S = 1, scalar: the same on the direct-write branch"),
    (((2, 4, 4, 4), (0, 0)), "S = 1, vector: one sweep, 248 idle threads"),
]
CS_ROLES = ('positive', 'cancelling', 'integer')


def cs_variants(C):
    return 1 if C >= 3 else -(-3 // C)


def cs_inputs(shape, v=0):
    """channel c plays CS_ROLES[(c + v) % 3]: all-positive values; values that cancel to (near) zero, so that only the bound
    against sum|x| holds them; signed integers below 2^24 / count, whose every partial sum is exact.  prev: what accumulate adds to
    (integers on the integer channels)"""
    N, C, H, W = shape
    n = N * H * W
    r = Q._rng(shape, 31 + v)
    x = np.empty(shape, np.float32)
    prev = r.randn(C).astype(np.float32)
    for c in range(C):
        k = CS_ROLES[(c + v) % 3]
        if k == 'positive':
            val = r.rand(n) + 0.5
        elif k == 'cancelling':
            val = r.randn(n).astype(np.float32)
            val[1::2] = -val[0:n - n % 2:2][r.permutation(n // 2)]
            if n % 2:
                val[-1] = 0.0
        else:
            b = (2 ** 24 - 1) // (n + 1)
            val = r.randint(-b, b + 1, n)
            prev[c] = r.randint(-b, b + 1)
        x[:, c] = np.asarray(val, np.float32).reshape(N, H, W)
    return dict(x=x, prev=prev)


def channel_sum(x, prev=None):
    """-> (sums, M) in float64"""
    x = np.asarray(x, np.float64)
    p = np.zeros(x.shape[1]) if prev is None else np.asarray(prev, np.float64)
    return x.sum(axis=(0, 2, 3)) + p, np.abs(x).sum(axis=(0, 2, 3)) + np.abs(p)


def _block32(t):
    """the block reduction of channel_sum_partial on the 256 per-thread fp32 sums: shuffles inside each wave, the LDS tree"""
    w = np.asarray(t, np.float32).reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :64 - o] = w[:, :64 - o] + w[:, o:]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def restate32_channel_sum(x, shape, spec, prev=None):
    """channel_sum_partial / channel_sum_final in float32 numpy, addition by addition in the kernels' order"""
    f = np.float32
    N, C, H, W = shape
    S, chunk, path = cs_dispatch(shape, spec)
    x = np.asarray(x, f)
    total = N * H * W
    out = np.empty(C, f)
    for c in range(C):
        flat = np.ascontiguousarray(x[:, c]).reshape(-1)            # element e of the channel: sample e / HW, position e % HW
        parts = []
        for s in range(S):
            run = flat[min(s * chunk, total):min(s * chunk + chunk, total)]
            if path == 'vector':
                sweeps = -(-max(run.size, 1) // 4096)
                pad = np.zeros(sweeps * 4096, f)
                pad[:run.size] = run
                u = pad.reshape(sweeps, 4, 256, 4)                  # [sweep][k][thread][lane of the float4]
                s4 = np.zeros((4, 256), f)
                for j in range(sweeps):
                    s4 = s4 + ((u[j, :, :, 0] + u[j, :, :, 1]) + (u[j, :, :, 2] + u[j, :, :, 3]))
                t = (s4[0] + s4[1]) + (s4[2] + s4[3])
            else:
                it = -(-max(run.size, 1) // 256)
                pad = np.zeros(it * 256, f)
                pad[:run.size] = run
                t = np.zeros(256, f)
                for j in range(it):
                    t = t + pad[j * 256:(j + 1) * 256]
            parts.append(_block32(t))
        acc = f(0)
        if S > 1:
            for p in parts:
                acc = f(acc + p)
        else:
            acc = parts[0]
        out[c] = f((f(prev[c]) if prev is not None else f(0)) + acc)
    return out


# ---- ghm_scale_samples ----
# ((N, C, H, W), view of x, extra elements between the samples of num and den)
SCALE_ROWS = [
    (((6, 3, 6, 10), (60, 120), 0), "VEC 4: the older test's shape, a channel slice of five channels"),
    (((3, 5, 7, 9), (0, 0), 0), "VEC 1: HW = 63"),
    (((2, 2, 2, 2), (0, 0), 2), "VEC 4: num / den at sample stride 3"),
]
DENORMAL = 1e-42


def scale_inputs(shape):
    """x, num, den; with N >= 3 the last three samples are: den = 0 behind an all-zero gradient (both signs of zero); den = 0
    behind zeros and ONE non-zero element (-> NaN there, the zeros stay); a denormal den behind a gradient that small.
    -> dict with ``nan``: the index of that element"""
    N, C, H, W = shape
    r = Q._rng(shape, 41)
    x = r.randn(*shape).astype(np.float32)
    num = (r.randn(N) + 0.1).astype(np.float32)
    den = (r.rand(N) + 0.25).astype(np.float32) * np.where(r.rand(N) < 0.5, -1, 1).astype(np.float32)
    nan = None
    if N >= 3:
        x[N - 3] = 0.0
        x[N - 3].reshape(-1)[::2] = -0.0
        x[N - 2] = 0.0
        x[N - 2].reshape(-1)[1::3] = -0.0
        nan = (N - 2, C - 1, H // 2, W - 1)
        x[nan] = 0.5
        x[N - 1] *= np.float32(1e-40)
        den[N - 3], den[N - 2], den[N - 1] = 0.0, 0.0, DENORMAL
    return dict(x=x, num=num, den=den, nan=nan)


def scale_samples(x, num, den):
    """x num / den in float64 where den != 0 -> (value, M = |value|); rows with den == 0 are the caller's"""
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(den != 0, np.asarray(num, np.float64) / np.asarray(den, np.float64), 0.0)
    v = np.asarray(x, np.float64) * ratio.reshape(-1, 1, 1, 1)
    return v, np.abs(v)


def restate32_scale_samples(x, num, den):
    return scale_samples(x, num, den)[0].astype(np.float32)


# ---- fp32 -> bf16 -> fp32 of the reduced-precision exchange ----
BF16_NS = (1, 255, 256, 257, 4099)
BF16_BITS = {
    'tie, even upper half': [0x3f808000, 0xbf808000, 0x40008000, 0x00028000],
    'tie, odd upper half': [0x3f818000, 0xbf818000, 0x7f7e8000, 0x00018000],
    'one ulp either side of a tie': [0x3f807fff, 0x3f808001, 0xbf817fff, 0xbf818001],
    'zeros': [0x00000000, 0x80000000],
    'denormals': [0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00007fff, 0x807f8000],
    'FLT_MAX': [0x7f7fffff, 0xff7fffff],
    'inf': [0x7f800000, 0xff800000],
    'quiet NaN': [0x7fc00000, 0xffc12345],
    'NaN, payload in the low half only': [0x7f800001, 0xff80ffff, 0x7f808000],
    'ordinary': [0x3f800000, 0x40490fdb, 0xc2f6e979, 0x3eaaaaab],
}


def bf16_inputs(n):
    """n fp32 bit patterns: the classes of BF16_BITS in turn, random bits behind them"""
    special = np.array(sum(BF16_BITS.values(), []), np.uint32)
    out = np.random.RandomState(n).randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    out[:min(n, special.size)] = np.roll(special, -(n % special.size))[:min(n, special.size)]
    return out


def rne_bf16_bits(u):
    """the upper halfword a correct conversion stores: oracle.lp.round_bf16 (nearest, ties to even; FLT_MAX -> inf; inf stays)
    for every non-NaN; a NaN keeps sign and upper payload and carries the quiet bit, so it is a NaN whatever its low half held"""
    u = np.asarray(u, np.uint32)
    x = u.view(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        r = LP.round_bf16(np.where(np.isnan(x), np.float32(0), x)).view(np.uint32) >> 16
    return np.where(np.isnan(x), (u >> 16) | 0x0040, r).astype(np.uint16)


def widen(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)
