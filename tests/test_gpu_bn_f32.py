"""The fp32 BatchNorm entry points of csrc/elementwise.hip (ghm_bn_stats / _apply / _forward / _backward / _backward_x) at
training batch sizes, ghm_channel_sum, ghm_scale_samples and the fp32 <-> bf16 kernels of ghm_allreduce_sum_bf16, row by row, at
the shapes of tests/bn_f32_ref.py's tables (each row says which branch of its launcher it reaches; tests/test_bn_f32_ref.py
checks those claims, the inputs and the bounds on the CPU).

Per call, the four points of tests/test_gpu_elementwise_f32.py:
  1. value: per element (per channel) |got - ref| <= k 2^-24 M against the float64 definition, k counted from the source
     (tests/bn_f32_ref.py); mean / inv against the two-pass statistics, inv with the fp64 conditioning term of E[x^2] - mu^2 in M
     (below one ulp, proven on the CPU); y against the definition from those statistics (K_IN_FWD) AND against the definition
     from the fp32 mean / inv the kernel stored (K_BN_APPLY); dx, dgamma, dbeta from the stored fp32 mean / inv / y; the running
     statistics from the stored fp32 mean / inv;
  2. bit identities: bn_forward == bn_stats then bn_apply in every output; bn_backward_x == bn_backward given the forward's y;
     accumulate == fl32(previous + increment) for dgamma / dbeta and for channel_sum on both of its branches; bn_stats without
     running statistics gives the same bits and leaves them alone; a kernel that converts gives the halfword of the definition;
  3. nothing else is written: every tensor, the per-channel vectors included, is a view inside a NaN-canary-filled allocation,
     no canary changes and the inputs are bit-unchanged;
  4. no element and no channel is left out of a comparison.

Measured on the MI355X, max over all rows of |got - ref| / (2^-24 M) against the k asserted, the rel-L2 where it is asserted
too, and the number of comparisons (the module prints the three when it finishes):
  bn_stats mean, inv      0.98 of 2; without running statistics the same bits          3.1e-08   120
  bn_running              1.87 of 5                                                    -         60
  bn_forward              2.20 of 6 / 6 / 7 (linear, relu / lrelu); tanh 1.90 of 6 (libm); every output == stats + apply
                                                                                       1.6e-07   894 / 8
  bn_apply                1.98 of 4 / 4 / 5 from the stored mean / inv; tanh 1.72 of 8 2.0e-07   90 / 6
  bn_backward             3.85 of 15; tanh 3.25 of 6 (libm)                            8.0e-08   90 / 6
  bn_dgamma / bn_dbeta    1.75 / 0.96 of 6 (tanh 8); accumulate exact fl32 sums        -         192 / 192
  bn_backward_x           dx, dgamma, dbeta == bn_backward's bit for bit               0         288
  channel_sum             5.64 of the row's chain (10 .. 271); integer channels and accumulate exact   -   51
  scale_samples           0.99 of 2                                                    2.6e-08   7
  bf16_exchange           the halfword of the definition bit for bit                   0         5
All 31 cases passed on their first run.  Two kernels were changed beforehand, both from reading the code and neither by a
failing row: channel_sum_partial takes its float4 loop only behind a 16-byte aligned pointer (the rows at an odd element now
take the scalar loop), and comm_f32_to_bf16_kernel sets the quiet bit of a NaN, whose payload in the low half alone used to be
cut off to an inf (the row 'NaN, payload in the low half only' holds it).
Wall time on the MI355X: this module 6.8 s, 6.2 s of it opening the one-rank communicator of the bf16 test (as
test_rccl_single_rank_allreduce does); the other 30 cases take 0.6 s.

Three rows of the table were asked for under another name and are kept under the one the arithmetic gives them, each with a
neighbour that reaches the branch meant: BatchNorm (3, 2, 43, 127) has 16383 values per channel and is the one-launch kernel
((3, 2, 43, 129) is the flat form with odd HW); channel_sum (3, 2, 64, 65) has HW = 4160 = 4 * 1040 and takes the float4 loop
((3, 2, 63, 65) is the scalar loop with S > 1 and a rounded chunk); channel_sum (1, 300, 64, 64) has S = 1 and so no final
kernel ((2, 257, 64, 64), 8.4 MB, runs two blocks of it).  The mean-1000 channel has spread 0.5, not 0.01: at 0.01 the fp64
conditioning term of inv is hundreds of ulp (tests/test_bn_f32_ref.py proves both).
"""
import ctypes
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import call, tuning_env
from tests import bn_f32_ref as R
from tests import canary
from tests import elementwise_q_ref as Q

pytestmark = pytest.mark.gpu

A = R.ALPHA
_REF = {}
LEDGER = canary.Ledger(lambda op, w, r, n: "measured %-22s worst k %7.3f  rel-L2 %.2e  (%d comparisons)" % (op, w, r, n))
gpu, mem = canary.fixtures(LEDGER, _REF, loss_scale=True)
cached = functools.partial(canary.cached, _REF)
V, clean, unchanged, fl32_sum = canary.View.free, canary.clean, canary.unchanged, canary.fl32_sum
note, exact = LEDGER.note, LEDGER.exact


def vec(v):
    return v.numpy().reshape(-1)


@pytest.mark.parametrize("row,why", R.BN_ROWS, ids=["%s-%s" % (r[0], r[1]) for r, _ in R.BN_ROWS])
def test_batchnorm(gpu, mem, row, why):
    """ghm_bn_stats, ghm_bn_apply, ghm_bn_forward, ghm_bn_backward and ghm_bn_backward_x on one row: every input set, every
    activation of the row"""
    dev, ops, D = gpu
    shape, vx, vy, vd, acts = R.row_views(row)
    N, C, H, W = shape
    one = N * H * W == 1
    L = R.bn_sum_chain(R.bn_dispatch(shape, vx, vy, vd, shape in R.NO_SMALL)['stats'], N, C, H * W)
    ws = dev.alloc(ops.bn_workspace(C))
    with tuning_env(**({"GHM_NO_BN_SMALL": "1"} if shape in R.NO_SMALL else {})):
        for v in range(R.variants(C)):
            d = cached(('bn', shape, v), lambda: R.bn_inputs(shape, v))
            roles = [R.role(c, v, C) for c in range(C)]
            plain = np.array([k != 'mean1000' for k in roles])
            tag = "%s set %d (%s)" % (shape, v, why.split(":")[0])
            x, dout = V(gpu, shape, vx, d['x']), V(gpu, shape, vd, d['dout'])
            gamma, beta = V(gpu, (C,), data=d['gamma']), V(gpu, (C,), data=d['beta'])
            # ---- statistics, with the running update ----
            mean, inv, rm, ri = V(gpu, (C,)), V(gpu, (C,)), V(gpu, (C,), data=d['run'][0]), V(gpu, (C,), data=d['run'][1])
            ops.bn_stats(x.t, mean.t, inv.t, ws, rm.t, ri.t, R.EPS, R.RUN_ALPHA)
            m32, i32 = vec(mean), vec(inv)
            mu, var, iv = cached(('stats', shape, v), lambda: R.bn_stats(d['x']))
            note('bn_stats', m32, mu, np.abs(mu) + 1e-30, tag + " mean", k=R.K_IN_STATS, rel_limit=False)
            note('bn_stats', i32, iv, R.inv_M(shape, mu, var, iv, L), tag + " inv", k=R.K_IN_STATS)
            for t, s32, j in ((rm, m32, 0), (ri, i32, 1)):
                ref, M = R.running(d['run'][j], s32)
                note('bn_running', vec(t), ref, M, tag + (" run_inv" if j else " run_mean"), k=R.K_RUN, rel_limit=False)
            if 'constant' in roles:
                c = roles.index('constant')
                assert m32[c] == np.float32(R.CONST) and i32[c] == np.float32(1 / np.sqrt(float(np.float32(R.EPS)))), tag
            mean.data, inv.data, rm.data, ri.data = mean.numpy(), inv.numpy(), rm.numpy(), ri.numpy()
            clean(tag, mean, inv, rm, ri)
            unchanged(tag, x)
            # ---- run_mean = NULL: the same bits, no trace ----
            mean2, inv2 = V(gpu, (C,)), V(gpu, (C,))
            ops.bn_stats(x.t, mean2.t, inv2.t, ws, None, None, R.EPS)
            exact('bn_stats', vec(mean2), m32, tag + " mean without running statistics")
            exact('bn_stats', vec(inv2), i32, tag + " inv without running statistics")
            clean(tag, mean2, inv2)
            unchanged(tag, x, rm, ri)
            for act in acts:
                what = tag + " " + act
                # ---- forward: one entry point == stats then apply ----
                y, y2 = V(gpu, shape, vy), V(gpu, shape, vy)
                mean3, inv3 = V(gpu, (C,)), V(gpu, (C,))
                rm3, ri3 = V(gpu, (C,), data=d['run'][0]), V(gpu, (C,), data=d['run'][1])
                ops.bn_forward(x.t, y.t, mean3.t, inv3.t, gamma.t, beta.t, ws, rm3.t, ri3.t, R.EPS, R.RUN_ALPHA, act, A)
                ops.bn_apply(x.t, y2.t, mean.t, inv.t, gamma.t, beta.t, act, A)
                y32 = y.numpy()
                for got, want, name in ((mean3, mean, "mean"), (inv3, inv, "inv"), (rm3, rm, "run_mean"), (ri3, ri, "run_inv")):
                    exact('bn_forward', vec(got), vec(want), what + " %s == bn_stats'" % name)
                exact('bn_forward', y32, y2.numpy(), what + " y == bn_apply's")
                yref, M, _, _, _ = cached(('fwd', shape, v, act), lambda: R.bn_forward(d['x'], d['gamma'], d['beta'], act, A))
                kf = R.K_LIBM['in_fwd_tanh'] if act == 'tanh' else R.K_IN_FWD[act]
                op = 'bn_forward/tanh' if act == 'tanh' else 'bn_forward'
                if plain.any():
                    note(op, y32[:, plain], yref[:, plain], M[:, plain], what, k=kf)
                if not plain.all():         # the fp32 mean of the mean-1000 channel is 3e-5 off: M holds it, rel-L2 cannot
                    note(op, y32[:, ~plain], yref[:, ~plain], M[:, ~plain], what + " mean-1000 channel", k=kf, rel_limit=False)
                y2ref, M2 = Q.bn_apply(d['x'], m32, i32, d['gamma'], d['beta'], act, A)
                note('bn_apply/tanh' if act == 'tanh' else 'bn_apply', y32, y2ref, M2, what + " from the stored mean / inv", k=Q.K_BN_APPLY[act])
                for c in range(C):          # variance 0: y = act(beta), whatever gamma
                    if one or roles[c] == 'constant':
                        want = Q.restate32_act(d['beta'][c:c + 1], act, A)[0] if act != 'tanh' else y32[0, c].flat[0]
                        exact('bn_forward', y32[:, c], np.full((N, H, W), want, np.float32), what + " channel %d: y = act(beta)" % c)
                clean(what, y, y2, mean3, inv3, rm3, ri3)
                unchanged(what, x, gamma, beta, mean, inv)
                y.data = y32
                # ---- backward from the forward's own y; the form without y; accumulate ----
                dx, dx2 = V(gpu, shape, vy), V(gpu, shape, vy)
                dg, db, dg2, db2 = V(gpu, (C,)), V(gpu, (C,)), V(gpu, (C,)), V(gpu, (C,))
                dg3, db3 = V(gpu, (C,), data=d['prev'][0]), V(gpu, (C,), data=d['prev'][1])
                ops.bn_backward(dout.t, y.t, x.t, dx.t, mean.t, inv.t, gamma.t, dg.t, db.t, ws, act, A)
                ops.bn_backward_x(dout.t, x.t, dx2.t, mean.t, inv.t, gamma.t, beta.t, dg2.t, db2.t, ws, act, A)
                ops.bn_backward_x(dout.t, x.t, dx2.t, mean.t, inv.t, gamma.t, beta.t, dg3.t, db3.t, ws, act, A, accumulate=True)
                ref, Mx, dgr, Mg, dbr, Mb = R.bn_backward(d['dout'], y32, d['x'], m32, i32, d['gamma'], act, A)
                dx32, g32, b32 = dx.numpy(), vec(dg), vec(db)
                note('bn_backward/tanh' if act == 'tanh' else 'bn_backward', dx32, ref, Mx, what, k=R.K_LIBM['in_bwd_tanh'] if act == 'tanh' else R.K_IN_BWD)
                note('bn_dgamma', g32, dgr, Mg, what, k=R.k_dgamma(act), rel_limit=False)
                note('bn_dbeta', b32, dbr, Mb, what, k=R.k_dgamma(act), rel_limit=False)
                if one:
                    assert not dx32.any(), (what, "one value per channel: dz - mean(dz) is exactly 0")
                exact('bn_backward_x', dx2.numpy(), dx32, what + " dx == bn_backward's")
                exact('bn_backward_x', vec(dg2), g32, what + " dgamma == bn_backward's")
                exact('bn_backward_x', vec(db2), b32, what + " dbeta == bn_backward's")
                exact('bn_dgamma', vec(dg3), fl32_sum(d['prev'][0], g32), what + " accumulate")
                exact('bn_dbeta', vec(db3), fl32_sum(d['prev'][1], b32), what + " accumulate")
                clean(what, dx, dx2, dg, db, dg2, db2, dg3, db3)
                unchanged(what, x, dout, y, gamma, beta, mean, inv)
                for t in (y, y2, dx, dx2):
                    dev.free(t.ptr)
            for t in (x, dout):
                dev.free(t.ptr)


@pytest.mark.parametrize("row,why", R.CS_ROWS, ids=["%s-%s" % r for r, _ in R.CS_ROWS])
def test_channel_sum(gpu, mem, row, why):
    """ghm_channel_sum per channel against sum|x|: both loops, S = 1 (direct write) and S > 1 (partials + final kernel), with and
    without accumulate on both, an exact answer on the integer channels"""
    dev, ops, D = gpu
    shape, spec = row
    C = shape[1]
    for v in range(R.cs_variants(C)):
        d = R.cs_inputs(shape, v)
        what = "%s %s set %d (%s)" % (shape, spec, v, why.split(":")[0])
        x, out = V(gpu, shape, spec, d['x']), V(gpu, (C,))
        ref, M = R.channel_sum(d['x'])
        ops.channel_sum(x.t, out.t, False)
        inc = vec(out)
        note('channel_sum', inc, ref, M, what, k=R.k_channel_sum(shape, spec, False), rel_limit=False)
        whole = np.array([R.CS_ROLES[(c + v) % 3] == 'integer' for c in range(C)])
        assert np.array_equal(inc[whole].astype(np.float64), ref[whole]), (what, "integer channels have an exact sum")
        clean(what, out)
        out.set(d['prev'])
        ops.channel_sum(x.t, out.t, True)
        acc = vec(out)
        exact('channel_sum', acc, fl32_sum(d['prev'], inc), what + " accumulate")
        note('channel_sum', acc, ref + d['prev'], M + np.abs(d['prev']), what + " accumulate", k=R.k_channel_sum(shape, spec, True), rel_limit=False)
        assert np.array_equal(acc[whole].astype(np.float64), (ref + d['prev'])[whole]), (what, "integer channels, accumulated")
        clean(what, out)
        unchanged(what, x)
        dev.free(x.ptr)


@pytest.mark.parametrize("row,why", R.SCALE_ROWS, ids=[str(r[0]) for r, _ in R.SCALE_ROWS])
def test_scale_samples_rows(gpu, mem, row, why):
    """ghm_scale_samples against the float64 product rounded once; den == 0 keeps exact zeros and makes anything else NaN"""
    dev, ops, D = gpu
    shape, vx, extra = row
    N = shape[0]
    d = R.scale_inputs(shape)
    x = V(gpu, shape, vx, d['x'])
    num, den = V(gpu, (N, 1, 1, 1), (0, extra), d['num']), V(gpu, (N, 1, 1, 1), (0, extra), d['den'])
    ops.scale_samples(x.t, num.t, den.t)
    got = x.numpy()
    ref, M = R.scale_samples(d['x'], d['num'], d['den'])
    live = d['den'] != 0
    note('scale_samples', got[live], ref[live], M[live], "%s (%s)" % (shape, why.split(":")[0]), k=R.K_SCALE)
    if N >= 3:
        assert (got[N - 3] == 0).all(), (shape, "den == 0 behind exact zeros stays zero")
        nan = np.zeros(shape[1:], bool)
        nan[d['nan'][1:]] = True
        assert np.isnan(got[N - 2][nan]).all() and (got[N - 2][~nan] == 0).all(), (shape, "den == 0: NaN where x != 0, 0 elsewhere")
        assert (got[N - 1][d['x'][N - 1] != 0] != 0).all(), (shape, "a denormal den is no zero")
        LEDGER.tally('scale_samples', 2)
    clean(shape, x)
    unchanged(shape, num, den)


def test_bf16_exchange_rounds_to_nearest_even(gpu, mem):
    """ghm_allreduce_sum_bf16 on a one-rank communicator returns widen(rne_bf16(x)) bit for bit: ties both ways, their
    neighbours, zeros, denormals, FLT_MAX -> inf, inf, and NaN -> NaN even with a payload in the low half alone"""
    dev, ops, D = gpu
    uid = (ctypes.c_uint8 * 128)()
    call("ghm_comm_unique_id", ctypes.byref(uid))
    call("ghm_comm_init", dev.h, 0, 1, ctypes.byref(uid))
    try:
        for n in R.BF16_NS:
            u = R.bf16_inputs(n)
            buf = V(gpu, (n,))
            dev.h2d(buf.t.ptr, u)
            halfwords = (n + 1) // 2 * 2 + 8
            sp = dev.alloc(2 * halfwords)
            R.Q.canary_fill(dev, sp, 2 * halfwords)
            ops.allreduce_sum_bf16(buf.t, n, sp)
            dev.sync()
            got = np.empty(n, np.uint32)
            dev.d2h(got, buf.t.ptr, 4 * n)
            want = R.rne_bf16_bits(u)
            nan = np.isnan(u.view(np.float32))
            assert np.isnan(got.view(np.float32)[nan]).all(), ("n = %d" % n, "a NaN came back as something else",
                                                                [hex(b) for b in u[nan][~np.isnan(got.view(np.float32)[nan])][:4]])
            exact('bf16_exchange', got.view(np.float32), R.widen(want), "n = %d" % n)
            inside = np.zeros(halfwords, bool)
            inside[:n] = True
            assert R.Q.canary_changed(dev, sp, 2 * halfwords, inside).size == 0, ("n = %d" % n, "written behind the scratch buffer")
            raw = np.empty(halfwords, np.uint16)
            dev.d2h(raw, sp, 2 * halfwords)
            assert np.array_equal(raw[:n], want), ("n = %d" % n, "the exchange buffer holds the rounded halfwords")
            clean("n = %d" % n, buf)
    finally:
        call("ghm_comm_destroy", dev.h)
