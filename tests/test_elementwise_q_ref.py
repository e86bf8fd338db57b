"""tests/elementwise_q_ref.py on the CPU: the float64 definitions against oracle/ops.py and torch autograd, the stored
halfwords of the four q dtypes, the branch every row of the shape tables claims to reach, and -- on every input set of
tests/test_gpu_elementwise_q.py -- that the kernels' expressions evaluated in plain float32 numpy stay inside the
per-element bounds the GPU module asserts.  A failure of the last group means a bound was chosen too tight, not that a
kernel is wrong."""
import numpy as np
import pytest

from oracle import lp as LP
from oracle import ops as O
from tests import elementwise_q_ref as R


def _is_bf16(a):
    return not (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0xffff).any()


# ---- the helper against the oracle and torch ----
@pytest.mark.parametrize("act", ['lrelu', 'relu', 'linear', 'tanh'])
def test_bn_forward_and_backward_against_oracle_and_autograd(act):
    torch = pytest.importorskip("torch")
    d = R.bn_inputs((3, 8, 5, 6))
    x, gamma, beta, dout = (d[k].astype(np.float64) for k in ('x', 'gamma', 'beta', 'dout'))
    y_o, mu, inv = O.bn_train_fwd(x, beta, gamma)
    assert np.allclose(mu, d['mean'], rtol=1e-6, atol=1e-7) and np.allclose(inv, d['inv'], rtol=1e-6)
    y, M = R.bn_apply(x, mu, inv, gamma, beta, act, R.ALPHA)
    fwd = {'lrelu': lambda v: O.lrelu_fwd(v, R.a32(R.ALPHA)), 'relu': O.relu_fwd, 'linear': lambda v: v, 'tanh': O.tanh_fwd}[act]
    assert np.allclose(y, fwd(y_o), rtol=1e-13, atol=1e-13) and (M >= np.abs(y_o) - 1e-12).all()
    dx, Mb, dg, db = R.bn_backward(dout, y, x, mu, inv, gamma, act, R.ALPHA)
    # oracle: the activation's vjp (from the pre-activation) in front of bn_train_vjp
    dz = {'lrelu': lambda: O.lrelu_vjp(y_o, R.a32(R.ALPHA), dout), 'relu': lambda: O.relu_vjp(y_o, dout), 'linear': lambda: dout,
          'tanh': lambda: O.tanh_vjp_from_out(y, dout)}[act]()
    dx_o, db_o, dg_o = O.bn_train_vjp(x, gamma, mu, inv, dz)
    assert np.allclose(dx, dx_o, rtol=1e-12, atol=1e-13) and np.allclose(dg, dg_o) and np.allclose(db, db_o)
    assert (Mb >= np.abs(dx) - 1e-12).all()
    # torch autograd through the batch statistics
    xt, gt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, gamma, beta))
    m = xt.mean(dim=(0, 2, 3), keepdim=True)
    v = xt.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    pre = (xt - m) / torch.sqrt(v + O.BN_EPS) * gt.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
    yt = {'lrelu': lambda t: torch.nn.functional.leaky_relu(t, R.a32(R.ALPHA)), 'relu': torch.relu, 'linear': lambda t: t,
          'tanh': torch.tanh}[act](pre)
    yt.backward(torch.tensor(dout))
    assert np.allclose(yt.detach().numpy(), y, rtol=1e-12, atol=1e-13)
    assert np.allclose(xt.grad.numpy(), dx, rtol=1e-9, atol=1e-11)
    assert np.allclose(gt.grad.numpy(), dg, rtol=1e-10) and np.allclose(bt.grad.numpy(), db, rtol=1e-10)


@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (2, 2), (3, 4), (8, 2), (5, 7)])
def test_bilinear_closed_form_literal_and_adjoint(hw):
    rng = np.random.RandomState(3)
    x = rng.randn(2, 3, *hw)
    y, M = R.bilinear(x)
    assert np.allclose(y, O.bilinear_up2_fwd(x), rtol=1e-14, atol=1e-14) and (M >= np.abs(y) - 1e-14).all()
    g = rng.randn(*y.shape)
    assert abs((y * g).sum() - (x * O.bilinear_up2_vjp(g)).sum()) < 1e-12 * (np.abs(y * g).sum() + 1)      # <U x, g> == <x, U^T g>


def test_interleave_is_the_stated_permutation_and_inverts():
    pp = np.arange(4 * 2 * 3 * 2 * 5, dtype=np.float64).reshape(8, 3, 2, 5)
    hi = R.pp_to_hi(pp)
    for n in range(2):
        for dy in range(2):
            for dx in range(2):
                assert np.array_equal(hi[n, :, dy::2, dx::2], pp[4 * n + 2 * dy + dx])
    assert np.array_equal(R.hi_to_pp(hi), pp)
    d = R.hi_inputs((1, 8, 2, 3))
    y, _ = R.bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], 'relu')
    assert np.array_equal(R.bn_apply_hi(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], 'relu')[0], R.pp_to_hi(y))
    a = R.bn_backward_hi(d['dhi'], y, d['x'], d['mean'], d['inv'], d['gamma'], 'relu')
    b = R.bn_backward(R.hi_to_pp(d['dhi']), y, d['x'], d['mean'], d['inv'], d['gamma'], 'relu')
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("act", R.ACTS)
def test_mask_backward_against_the_pooling_oracle(act):
    """a mask built from a real max-pool reproduces oracle.ops.maxpool_vjp followed by the activation's vjp, with the slope
    from y and from the sign bit"""
    rng = np.random.RandomState(4)
    pre = rng.randn(2, 8, 6, 8)
    pre[0, 0, :2, :2] = 0.75                            # a four-way tie
    a = R.act_fwd(pre, act, R.ALPHA)
    y = O.maxpool_fwd(a, 2)
    win = a.reshape(2, 8, 3, 2, 4, 2).transpose(0, 1, 2, 4, 3, 5).reshape(2, 8, 3, 4, 4)
    mask = sum(((win[..., b] == y).astype(np.uint8) << b) for b in range(4)) | ((y > 0).astype(np.uint8) << 4)
    assert (mask & 15 == 15).any()
    dy = rng.randn(*y.shape)
    ref = O.maxpool_vjp(a, y, dy, 2) * R.dact_from_out(a, act, R.ALPHA)
    for yy in (y, None):
        dx, M, db = R.mask_bwd(mask, yy, dy, act, R.ALPHA)
        assert np.allclose(dx, ref, rtol=1e-14, atol=0) and np.allclose(db, ref.sum(axis=(0, 2, 3)))


# ---- pieces() ----
def test_pieces_round_trip():
    rng = np.random.RandomState(5)
    a = (rng.randn(4096) * np.exp(rng.randn(4096) * 6).clip(1e-30, 1e3)).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.0, -2.0 ** -20]
    p3 = R.pieces(a, 'bf16x3')
    assert len(p3) == 3 and all(_is_bf16(p) for p in p3)
    assert R.bits_equal(sum(p.astype(np.float64) for p in p3).astype(np.float32) + np.float32(0), a + np.float32(0))
    assert np.array_equal(sum(p.astype(np.float64) for p in p3), a.astype(np.float64))
    p2 = R.pieces(a, 'bf16x2')
    assert len(p2) == 2 and all(_is_bf16(p) for p in p2) and R.bits_equal(p2[0], p3[0]) and R.bits_equal(p2[1], p3[1])
    assert (np.abs(a.astype(np.float64) - p2[0] - p2[1]) <= 2.0 ** -17 * np.abs(a.astype(np.float64))).all()
    assert R.bits_equal(R.pieces(a, 'bf16')[0], LP.round_bf16(a)) and _is_bf16(R.pieces(a, 'bf16')[0])
    assert R.bits_equal(R.pieces(a, 'f16')[0], LP.round_f16(a))
    c = np.array([R.CANARY], np.uint16)
    assert np.isnan(c.view(np.float16)[0]) and np.isnan((c.astype(np.uint32) << 16).view(np.float32)[0])
    assert np.isnan(np.array([R.CANARY, R.CANARY], np.uint16).view(np.float32)[0])


def test_canary_masks():
    m = R.q_inside(2, 2, 10, 20, 3, 4, 45)
    assert m.sum() == 2 * 2 * 4 * 8 and m[3 * 8] and not m[7 * 8] and m[(20 + 10 + 3) * 8] and not m[40 * 8:].any()
    f = R.f32_inside(2, 10, 2, 5, 20)
    assert f.sum() == 2 * 5 * 2 and f[4] and not f[3] and f[(10 + 6) * 2 + 1] and not f[(10 + 7) * 2]


# ---- the tables reach what they say ----
def test_shape_tables_reach_the_branches_they_name():
    bn = {s: R.bn_sums_dispatch(s[0], s[1], s[2] * s[3]) for s, _ in R.BN_ROWS}
    assert bn[(3, 24, 10, 12)] == ('rows', 3) and bn[(1, 16, 5, 6)] == ('flat', 1) and bn[(2, 8, 3, 10)] == ('flat', 1)
    assert bn[(2, 16, 64, 64)] == ('rows', 4) and bn[(2, 16, 45, 46)] == ('flat', 2) and bn[(2, 64, 128, 128)] == ('rows', 16)
    assert bn[(3, 8, 1, 2)] == ('flat', 1)
    assert any(N * (C // 8) * H * W % 256 for (N, C, H, W), _ in R.BN_ROWS)                       # the tail of q_decode
    assert any((C // 8) * H * W > 2 ** 16 for (N, C, H, W), _ in R.BN_ROWS)
    assert {(1, 1), (1, 3), (2, 2), (3, 4), (8, 2), (32, 32)} <= {s[2:] for s, _ in R.COARSE_ROWS}
    hi = {s: R.bn_hi_split(*s) for s, _ in R.HI_BWD_ROWS}
    assert hi[(3, 16, 21, 17)] == (2, [536, 535]) and hi[(2, 512, 32, 32)] == (4, [512] * 4)
    assert hi[(3, 24, 10, 12)][0] == 1 and hi[(2, 8, 1, 1)][0] == 1
    assert (2048 + 511) // 512 == 4 and 2048 // 512 == 4                                         # the two caps meet
    pool = {s: (R.pool_bpp(s[2], s[3], False), R.pool_bpp(s[2], s[3], True)) for s, _ in R.POOL_ROWS}
    assert pool[(2, 16, 36, 20)][0] == (360, 2) and pool[(2, 16, 72, 40)][1] == (360, 2) and pool[(2, 16, 72, 40)][0] == (1440, 6)
    assert pool[(1, 8, 2, 4)] == ((4, 1), (1, 1)) and pool[(3, 24, 20, 28)] == ((280, 2), (70, 1))
    assert pool[(2, 64, 128, 128)] == ((8192, 32), (2048, 8))
    for rows in (R.BN_ROWS, R.COARSE_ROWS, R.HI_BWD_ROWS, R.POOL_ROWS):
        assert any(s[1] == 8 for s, _ in rows) and any(s[0] == 1 for s, _ in rows) or rows is R.HI_BWD_ROWS
        assert all(s[1] % 8 == 0 and why for s, why in rows)
    assert all(s[2] * s[3] % 2 == 0 for s, _ in R.BN_ROWS)                                        # what GHM_CHECK accepts
    assert all(s[2] % 2 == 0 and s[3] % 4 == 0 for s, _ in R.POOL_ROWS)


def test_pool_masks_hold_the_nibbles_the_issue_names():
    for s, _ in R.POOL_ROWS:
        d = R.pool_inputs(s)
        nib = d['mask'] & 15
        if nib.size >= 6:
            assert all((nib == v).any() for v in (15, 1, 2, 4, 8, 0))
        assert np.array_equal((d['mask'] & 16) != 0, d['y'] > 0) and not (d['mask'] >> 5).any()


# ---- fp32 arithmetic stays inside the bounds on the GPU module's inputs ----
def _acts_for(shape, acts):
    return acts if np.prod(shape) <= R.BIG else acts[:1]


@pytest.mark.parametrize("shape", [s for s, _ in R.BN_ROWS], ids=str)
def test_fp32_restatement_of_batchnorm_is_inside_the_bounds(shape):
    d = R.bn_inputs(shape)
    for act in _acts_for(shape, R.ACTS + ('tanh',)):
        y, M = R.bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, R.ALPHA)
        y32 = R.restate32_bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, R.ALPHA)
        assert R.worst(y32, y, M) <= R.K_BN_APPLY[act] and R.rel(y32, y) <= R.REL_L2, (act, R.worst(y32, y, M))
        if act == 'tanh':
            continue
        dx, Mb, dg, db = R.bn_backward(d['dout'], y32, d['x'], d['mean'], d['inv'], d['gamma'], act, R.ALPHA)
        dx32 = R.restate32_bn_backward(d['dout'], y32, d['x'], d['mean'], d['inv'], d['gamma'], act, R.ALPHA)
        assert R.worst(dx32, dx, Mb) <= R.K_BN_BWD and R.rel(dx32, dx) <= R.REL_L2, (act, R.worst(dx32, dx, Mb))


@pytest.mark.parametrize("shape", [s for s, _ in R.HI_BWD_ROWS] + [s for s, _ in R.COARSE_ROWS], ids=str)
def test_fp32_restatement_of_the_interleaved_batchnorm_is_inside_the_bounds(shape):
    d = R.hi_inputs(shape)
    for act in _acts_for((4,) + shape, R.ACTS + ('tanh',)):
        y, M = R.bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, R.ALPHA)
        y32 = R.restate32_bn_apply(d['x'], d['mean'], d['inv'], d['gamma'], d['beta'], act, R.ALPHA)
        assert R.worst(y32, y, M) <= R.K_BN_APPLY[act]
        if act == 'tanh':
            continue
        dx, Mb, dg, db = R.bn_backward_hi(d['dhi'], y32, d['x'], d['mean'], d['inv'], d['gamma'], act, R.ALPHA)
        dx32 = R.restate32_bn_backward(R.hi_to_pp(d['dhi']), y32, d['x'], d['mean'], d['inv'], d['gamma'], act, R.ALPHA)
        assert R.worst(dx32, dx, Mb) <= R.K_BN_BWD and R.rel(dx32, dx) <= R.REL_L2, (act, R.worst(dx32, dx, Mb))


@pytest.mark.parametrize("shape", [s for s, _ in R.COARSE_ROWS], ids=str)
def test_fp32_restatement_of_bilinear_is_inside_the_bounds(shape):
    x = R.bn_inputs(shape)['x']
    y, M = R.bilinear(x)
    y32 = R.restate32_bilinear(x)
    assert y32.dtype == np.float32 and R.worst(y32, y, M) <= R.K_BILINEAR and R.rel(y32, y) <= R.REL_L2


@pytest.mark.parametrize("shape", [s for s, _ in R.POOL_ROWS], ids=str)
def test_fp32_restatement_of_the_mask_backward_is_inside_the_bounds(shape):
    d = R.pool_inputs(shape)
    for act in R.ACTS:
        for y in (d['y'], None):
            dx, M, db = R.mask_bwd(d['mask'], y, d['dy'], act, R.ALPHA)
            dx32 = R.restate32_mask_bwd(d['mask'], y, d['dy'], act, R.ALPHA)
            assert dx32.dtype == np.float32 and R.worst(dx32, dx, M) <= R.K_MASK_BWD
        a, b = R.mask_bwd(d['mask'], d['y'], d['dy'], act, R.ALPHA), R.mask_bwd(d['mask'], None, d['dy'], act, R.ALPHA)
        assert np.array_equal(a[0], b[0])                       # the sign bit says what y says
