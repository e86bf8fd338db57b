"""tests/elementwise_f32_ref.py on the CPU: every row of the shape tables reaches the branch its note names under the restated
launcher arithmetic, and every branch of the launchers is reached by some row; the input sets hold the ties, zeros and borders
they are meant to hold; the float64 definitions agree with oracle/ops.py, with each other (adjoint identities) and with the two
documented differences from Theano; and the kernels' expressions evaluated in plain float32 numpy stay inside the per-element
bounds the GPU module asserts, on that module's own inputs.  A failure of the last group means a bound was chosen too tight,
not that a kernel is wrong."""
import numpy as np
import pytest

from oracle import ops as O
from tests import elementwise_f32_ref as R
from tests import elementwise_q_ref as Q

A = R.ALPHA


# ---- the tables reach what they say ----
def _starts(note, word):
    return note.startswith(word + ":") or note.startswith(word + " ")


def test_loss_rows_reach_single_multi_and_capped_grids():
    assert [R.loss_grid(n) for n in (1, 2048, 2049, 2 ** 21, 2 ** 21 + 1, 2 ** 30)] == [1, 1, 2, 1024, 1024, 1024]
    for n, note in R.LOSS_NS:
        assert _starts(note, R.loss_path(n)), (n, note, R.loss_path(n))
    assert {R.loss_path(n) for n, _ in R.LOSS_NS} == {'single', 'multi', 'capped'}
    assert {1, 2047, 2048, 2049, 16384, 2 ** 21 + 5} <= {n for n, _ in R.LOSS_NS}
    assert all(n < 2 ** 24 for n, _ in R.LOSS_NS)                       # (float)n is exact


def test_recon_rows_reach_both_vec_widths_sliced_and_the_grid_cap():
    seen = set()
    for (shape, l2, va, vb, vg, gs), note in R.RECON_ROWS:
        N, C, H, W = shape
        views = [R.view_of(shape, v) for v in (va, vb, vg)]
        vec, path = R.recon_path(N, C, H * W, *views)
        assert note.startswith("VEC %d, %s:" % (vec, path)), (shape, note, vec, path)
        sliced = len({ns for _, ns in views}) == 3
        seen.add((vec, path, l2, sliced))
        assert N * C * H * W < 2 ** 24
    assert {(v, p) for v, p, _, _ in seen} >= {(4, 'single'), (1, 'single'), (4, 'multi'), (1, 'multi'), (4, 'capped')}
    assert {(v, s) for v, _, _, s in seen} >= {(4, True), (1, True)}         # three different strides on both widths
    assert {l2 for _, _, l2, _ in seen} == {False, True}
    # C HW % 4 == 0 alone does not give VEC 4
    assert R.recon_vec(4, 64, (0, 256), (2, 260), (0, 256)) == 1 and R.recon_vec(4, 64, (0, 256), (4, 260), None) == 4


def test_upsample_rows_reach_both_adjoint_kernels_for_every_reason():
    seen = set()
    for (shape, vx, vd, big), note in R.UP_ROWS:
        N, C, H, W = shape
        kern, what = R.bilinear_bwd_kernel(N, C, H, W, R.view_of(shape, vd))
        assert note.startswith("%s x %d:" % (kern, what) if kern == 'bwd2' else "slow: %s" % what), (shape, note, kern, what)
        seen.add((kern, what))
    assert seen >= {('slow', 'odd W'), ('slow', 'odd dxs'), ('slow', 'dx 4-byte aligned'), ('slow', 'N C > 65535'), ('bwd2', 1), ('bwd2', 2)}
    shapes = [r[0][0] for r in R.UP_ROWS]
    assert any(s[2] == 1 for s in shapes) and any(s[3] % 2 for s in shapes) and any(s[3] % 2 == 0 for s in shapes)
    assert any(s[0] * s[1] == 65535 for s in shapes) and any(s[0] * s[1] > 65535 for s in shapes)
    sliced = [(r[0][0], r[0][2]) for r in R.UP_ROWS if r[0][2] != (0, 0)]
    assert any(R.bilinear_bwd_kernel(*s, R.view_of(s, v))[0] == 'bwd2' for s, v in sliced)     # a slice on the fast kernel too
    assert {v[0] % 2 for _, v in sliced} == {0, 1}                                              # even and odd slice offsets


def test_pool_rows_reach_the_geometries():
    per = {s: (s[2] // 2) * (s[3] // 2) for s, _ in R.MAXPOOL_ROWS}
    assert any(v > 256 for v in per.values())
    assert any(v < 256 and s[0] * s[1] * v > 256 and 256 % v for s, v in per.items())          # a block boundary inside a plane
    assert any(s[2] == 2 for s in per) and any(s[3] == 2 for s in per)
    assert all(s[2] % 2 or s[3] % 2 for s in R.MAXPOOL_REFUSED) and {s[2] % 2 for s in R.MAXPOOL_REFUSED} == {0, 1}
    ps = {(p, s[2] == p and s[3] == p, bool(s[2] % p), bool(s[3] % p)) for (s, p), _ in R.AVGPOOL_ROWS}
    assert {p for p, _, _, _ in ps} == {2, 4, 8}
    assert any(g for _, g, _, _ in ps) and any(h and w for _, _, h, w in ps)
    assert any(s[0] * s[1] * s[2] * s[3] > 256 for (s, p), _ in R.AVGPOOL_ROWS)


def test_grad_check_rows_reach_body_sweep_and_tail():
    assert R.grad_check_grid(2 ** 21) == (2048, 2 ** 19, False, 0) and R.grad_check_grid(2 ** 21 - 4)[0] == 2048
    assert R.grad_check_grid(2 ** 21 - 1024)[0] == 2047
    want = {1: (1, 0, False, 1), 3: (1, 0, False, 3), 4: (1, 1, False, 0), 5: (1, 1, False, 1), 1023: (1, 255, False, 3),
            2 ** 21 + 7: (2048, 2 ** 19 + 1, True, 3)}
    for n, note in R.GRAD_CHECK_NS:
        g = R.grad_check_grid(n)
        assert g == want[n], (n, g)
        assert note.startswith("%d block" % g[0]) and ("second grid sweep" in note) == g[2], (n, note)
        assert ("no tail" in note) == (g[3] == 0) and ("no float4" in note) == (g[1] == 0)
        pos = R.grad_check_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= p < n for p in pos)
        assert {4 * g[1] + t for t in range(g[3])} <= set(pos)                                   # every tail position
    assert max(R.grad_check_positions(2 ** 21 + 7)) > 2097152 and 2097152 in R.grad_check_positions(2 ** 21 + 7)
    bits = np.array(R.NONFINITE, np.uint32).view(np.float32)
    assert np.isposinf(bits[0]) and np.isneginf(bits[1]) and np.isnan(bits[2:]).all() and (np.array(R.NONFINITE[3:]) & 0x3fffff).all()
    assert np.isfinite(np.array(R.FINITE_EXTREMES, np.uint32).view(np.float32)).all()
    assert np.isnan(np.array([R.Q.CANARY | (R.Q.CANARY << 16)], np.uint32).view(np.float32)[0])   # what lies behind n is a NaN


def test_instance_norm_rows_reach_the_one_launch_and_three_pass_forms():
    seen, acts, groups, accs = set(), set(), set(), set()
    for (shape, group, act, vx, vy, acc), note in R.IN_ROWS:
        N, C, H, W = shape
        assert N % group == 0
        d = R.in_dispatch(group, C, H * W, [R.view_of(shape, vx), R.view_of(shape, vy)])
        want = "small %d:" % d[1] if d[0] == 'small' else d[0] + ":"
        assert note.startswith(want), (shape, note, d)
        if d[0] != 'small':
            assert "S = %d" % d[1] in note and ("VEC %d" % d[2] in note), (shape, note, d)
        seen.add((d[0], d[-1], group > 1, N // group > 1, (vx, vy) != ((0, 0), (0, 0))))
        acts.add(act), groups.add(group), accs.add(acc)
    forms = {(f, v) for f, v, _, _, _ in seen}
    assert forms >= {('small', 4), ('small', 1), ('rows', 4), ('flat', 1)}
    assert {(f, g) for f, _, g, _, _ in seen} >= {('small', True), ('rows', True)}                 # group > 1 on both forms
    assert {(f, s) for f, _, _, _, s in seen} >= {('small', True), ('rows', True)}                 # slices on both forms
    assert any(f != 'small' and many for f, _, _, many, _ in seen)                                 # several three-pass instances
    assert acts == {'lrelu', 'relu', 'linear', 'tanh'} and groups == {1, 2} and accs == {False, True}
    hw = {r[0][0][2] * r[0][0][3] for r in R.IN_ROWS}
    assert hw >= {256, 16384, 16388, 65536, 16383, 16385} and {r[0][0][1] for r in R.IN_ROWS} == {3, 64}
    assert R.bn_small(16384) and not R.bn_small(16385) and R.IN_REFUSED[0][0] % R.IN_REFUSED[1]
    # the same arithmetic as elementwise_q_ref's restatement of ghm_bn_backward_sums
    for (shape, group, act, vx, vy, acc), _ in R.IN_ROWS:
        d = R.in_dispatch(group, shape[1], shape[2] * shape[3], [R.view_of(shape, vx), R.view_of(shape, vy)])
        if d[0] != 'small':
            assert Q.bn_sums_dispatch(group, shape[1], shape[2] * shape[3], d[2] == 4) == d[:2]


def test_optimizer_rows_reach_the_float4_body_and_the_tail():
    assert {n % 4 for n, _ in R.OPT_NS} >= {0, 1, 3} and all(n >= 4 for n, _ in R.OPT_NS)
    assert R.RMSPROP_CONSTS != (0.9, 1e-6) and R.ADAM_CONSTS != (0.9, 0.999, 1e-8) and R.ADAM_T0 == (0.0, 1e5)


# ---- the inputs hold what they are meant to hold ----
def test_maxpool_inputs_tie_in_every_pattern():
    counts, mixed_zero, const = set(), False, False
    for shape, _ in R.MAXPOOL_ROWS:
        x = R.maxpool_inputs(shape)['x']
        w = R.windows(x)
        eq = w == w.max(-1, keepdims=True)
        counts |= set(np.unique(eq.sum(-1)).tolist())
        sign = np.signbit(w)
        mixed_zero |= bool(((w.max(-1) == 0) & (eq & sign).any(-1) & (eq & ~sign).any(-1)).any())
        const |= bool((x[0, 0] == x[0, 0, 0, 0]).all())
        assert (eq.sum(-1) > 1).mean() > 0.5                          # most windows tie
        patterns = {tuple(e) for e in eq.reshape(-1, 4)}
        assert len(patterns) >= 8 or w.size < 200
    assert counts == {1, 2, 3, 4} and mixed_zero and const
    # every one of the fifteen tie patterns occurs somewhere in the table
    allp = set()
    for shape, _ in R.MAXPOOL_ROWS:
        w = R.windows(R.maxpool_inputs(shape)['x'])
        allp |= {tuple(e) for e in (w == w.max(-1, keepdims=True)).reshape(-1, 4)}
    assert len(allp) == 15


def test_known_differences_from_theano_are_pinned():
    """the LeakyReLU slope at an output of exactly 0 is alpha, not Theano's (1 + alpha) / 2; sign(0) = 0 in L1 (Theano agrees on
    the value, its gradient of abs at 0 is 0 too -- the kernel spells the case out)"""
    x = np.array([[[[0.0, -1.0], [-0.0, -2.0]]]], np.float32)
    y = R.maxpool_fwd(x)
    dx, _ = R.maxpool_bwd(x, y, np.ones((1, 1, 1, 1), np.float32), 'lrelu', A)
    assert np.array_equal(dx, np.array([[[[R.a32(A), 0], [R.a32(A), 0]]]]))
    theano = O.lrelu_vjp(x.astype(np.float64), R.a32(A), O.maxpool_vjp(x.astype(np.float64), y, np.ones((1, 1, 1, 1)), 2))
    assert np.allclose(theano[0, 0, :, 0], 0.5 * (1 + R.a32(A)))
    assert np.array_equal(R.maxpool_bwd(x, y, np.ones((1, 1, 1, 1), np.float32), 'relu')[0], np.zeros((1, 1, 2, 2)))
    for (shape, l2, va, vb, vg, gs), _ in R.RECON_ROWS[:3]:
        d = R.recon_inputs(shape)
        eq = d['a'] == d['b']
        assert 0.05 < eq.mean() < 0.25
        loss, g, M = R.recon_loss(d['a'], d['b'], l2, gs)
        assert (g[eq] == 0).all() and (g[~eq] != 0).all()
        l32, g32 = R.restate32_recon_loss(d['a'], d['b'], l2, gs)
        assert (g32[eq] == 0).all()
    for shape, _ in R.MAXPOOL_ROWS:                                    # the pooling inputs hit the zero output with every slope
        d = R.maxpool_inputs(shape)
        y = R.maxpool_fwd(d['x'])
        assert (y == 0).any()
        hit = (d['x'] == 0) & (y.repeat(2, 2).repeat(2, 3) == 0)
        dx, _ = R.maxpool_bwd(d['x'], y, d['dy'], 'lrelu', A)
        gu = d['dy'].astype(np.float64).repeat(2, 2).repeat(2, 3)
        assert hit.any() and np.array_equal(dx[hit], (gu * R.a32(A))[hit])


# ---- the float64 definitions ----
def test_maxpool_and_avgpool_definitions():
    for shape, _ in R.MAXPOOL_ROWS:
        d = R.maxpool_inputs(shape)
        y = R.maxpool_fwd(d['x'])
        assert R.maxpool_selects(y.astype(np.float32), d['x'])
        bad = y.astype(np.float32).copy()
        bad.reshape(-1)[0] += 1
        assert not R.maxpool_selects(bad, d['x'])
        dx, M = R.maxpool_bwd(d['x'], y, d['dy'], 'linear')
        assert np.allclose(dx.reshape(shape[0], shape[1], shape[2] // 2, 2, shape[3] // 2, 2).sum(axis=(3, 5)),
                           d['dy'] * (R.windows(d['x']) == y[..., None]).sum(-1))
    for (shape, p), _ in R.AVGPOOL_ROWS:
        x = Q.view_inputs(shape)['x']
        y, M = R.avgpool_fwd(x, p)
        g = np.random.RandomState(1).randn(*y.shape)
        dx, _ = R.avgpool_bwd(shape, g, p)
        assert abs((y * g).sum() - (x.astype(np.float64) * dx).sum()) < 1e-12 * (np.abs(y * g).sum() + 1)
        Ho, Wo = shape[2] // p, shape[3] // p
        assert (dx[:, :, Ho * p:] == 0).all() and (dx[:, :, :, Wo * p:] == 0).all()
        x2 = x.copy()
        x2[:, :, Ho * p:], x2[:, :, :, Wo * p:] = 1e6, -1e6            # the border is ignored forward
        assert np.array_equal(R.avgpool_fwd(x2, p)[0], y)


@pytest.mark.parametrize("row", [r for r, _ in R.UP_ROWS], ids=lambda r: "%s-%s" % (r[0], r[2]))
def test_adjoint_identities_and_the_two_bilinear_definitions(row):
    shape = row[0]
    d = R.up_inputs(shape)
    x, g = d['x'].astype(np.float64), d['g'].astype(np.float64)
    lit, closed, M = R.bilinear_fwd(d['x'])
    assert np.allclose(lit, closed, rtol=1e-14, atol=1e-14) and (M >= np.abs(lit) - 1e-14).all()
    for up, adj in ((closed, R.bilinear_bwd(d['g'])[0]), (R.nearest_fwd(x), R.nearest_bwd(d['g'])[0])):
        lhs, rhs = (up * g).sum(), (x * adj).sum()                     # <up(x), g> == <x, up^T(g)>
        assert abs(lhs - rhs) <= 1e-11 * (np.abs(up * g).sum() + 1), (lhs, rhs)


def test_instance_norm_definition_against_the_oracle_and_by_groups():
    torch = pytest.importorskip("torch")
    shape, group = (4, 3, 5, 6), 2
    d = R.in_inputs(shape, group)
    x, dout, gamma, beta = (d[k].astype(np.float64) for k in ('x', 'dout', 'gamma', 'beta'))
    for act in ('lrelu', 'tanh', 'linear', 'relu'):
        y, M, mu, inv = R.instance_norm_fwd(d['x'], d['gamma'], d['beta'], act, A, group)
        # the definition of a group: the statistics of torch's instance norm over the concatenated maps
        xt = torch.tensor(R.to_groups(x, group), requires_grad=True)
        gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
        pre = torch.nn.functional.instance_norm(xt, weight=gt, bias=bt, eps=float(np.float32(R.IN_EPS)))
        yt = {'lrelu': lambda t: torch.nn.functional.leaky_relu(t, R.a32(A)), 'tanh': torch.tanh, 'linear': lambda t: t,
              'relu': torch.relu}[act](pre)
        assert np.allclose(R.to_groups(y, group), yt.detach().numpy(), rtol=1e-11, atol=1e-12)
        yt.backward(torch.tensor(R.to_groups(dout, group)))
        dx, Mx, dg, Mg, db, Mb = R.instance_norm_bwd(dout, y, x, mu, inv, gamma, act, A, group)
        assert np.allclose(R.to_groups(dx, group), xt.grad.numpy(), rtol=1e-8, atol=1e-10)
        assert np.allclose(dg, gt.grad.numpy(), rtol=1e-9) and np.allclose(db, bt.grad.numpy(), rtol=1e-9)
        assert (Mx >= np.abs(dx) - 1e-12).all() and (Mg >= np.abs(dg) - 1e-9).all() and (Mb >= np.abs(db) - 1e-9).all()
    # group 1 is oracle.ops.in_fwd / in_vjp itself
    y, M, mu, inv = R.instance_norm_fwd(d['x'], d['gamma'], d['beta'], 'linear')
    yo, muo, invo = O.in_fwd(x, beta, gamma, float(np.float32(R.IN_EPS)))
    assert np.array_equal(y, yo) and np.array_equal(mu, muo)
    dx, _, dg, _, db, _ = R.instance_norm_bwd(dout, y, x, mu, inv, gamma, 'linear')
    dxo, dbo, dgo = O.in_vjp(x, gamma, mu, inv, dout)
    assert np.allclose(dx, dxo, rtol=1e-12, atol=1e-13) and np.allclose(dg, dgo) and np.allclose(db, dbo)
    assert np.array_equal(R.from_groups(R.to_groups(x, 2), 2), x)
    # the constant plane: var = 0, inv = 1 / sqrt(eps), y = act(beta)
    assert np.allclose(inv[0, -1], 1 / np.sqrt(float(np.float32(R.IN_EPS)))) and np.allclose(y[0, -1], beta[-1], atol=1e-12)


def test_losses_and_updates_are_the_oracles():
    d = R.loss_inputs(2049, 'bce')
    assert 0.1 <= d.min() and d.max() <= 0.9
    for kind, fn in (('lsgan', O.squared_error_mean), ('bce', O.bce_mean)):
        d = R.loss_inputs(2049, kind)
        for t in (0.0, 1.0):
            loss, Ml, g, Mg = R.scalar_loss(d, t, kind, 0.5)
            lo, go = fn(d.astype(np.float64), t)
            assert loss == lo and np.array_equal(g, 0.5 * go) and Ml >= abs(loss) * (1 - 1e-12)
    n = 1003
    d = {k: v.astype(np.float64) for k, v in R.opt_inputs(n).items()}
    p2, _, a2, _ = R.rmsprop(d['p'], d['g'], d['acc'], 1e-2, *R.RMSPROP_CONSTS, 0.5)
    rho, eps = R.f64(*R.RMSPROP_CONSTS)
    gg = 0.5 * d['g']
    acc = rho * d['acc'] + (1 - rho) * gg * gg
    assert np.allclose(a2, acc, rtol=1e-14) and np.allclose(p2, d['p'] - R.f64(1e-2)[0] * gg / np.sqrt(acc + eps), rtol=1e-13)
    p3, _, m3, _, v3, _ = R.adam(d['p'], d['g'], d['m'], d['acc'], 4.0, 1e-2, *R.ADAM_CONSTS, 0.5)
    b1, b2, eps = R.f64(*R.ADAM_CONSTS)
    m, v = b1 * d['m'] + (1 - b1) * gg, b2 * d['acc'] + (1 - b2) * gg * gg
    a_t = R.f64(1e-2)[0] * np.sqrt(1 - b2 ** 5) / (1 - b1 ** 5)
    assert np.allclose(m3, m, rtol=1e-14) and np.allclose(v3, v, rtol=1e-14) and np.allclose(p3, d['p'] - a_t * m / (np.sqrt(v) + eps), rtol=1e-12)


def test_loss_scale_state_machine_runs_reach_floor_cap_and_both_branches():
    for interval, lo, hi, s0, flags in R.LOSS_SCALE_RUNS[:1]:
        ls = np.array([s0, 1 / s0, 0, 0, 0, 0, 0, 0], np.float32)
        floor = cap = grew = 0
        for f in flags:
            before = ls.copy()
            ls[3] = f
            ls = R.loss_scale_update(ls, interval, lo, hi)
            assert ls[3] == 0 and ls[1] == np.float32(1) / ls[0] and (ls[5:] == 0).all()
            if f:
                assert ls[2] == 0 and ls[4] == before[4] + 1 and ls[0] == max(before[0] / 2, np.float32(lo))
                floor += before[0] / 2 < lo
            else:
                assert ls[4] == before[4]
                if before[2] + 1 >= interval:
                    assert ls[0] == min(before[0] * 2, np.float32(hi)) and ls[2] == 0
                    grew += 1
                    cap += before[0] * 2 > hi
                else:
                    assert ls[0] == before[0] and ls[2] == before[2] + 1
        assert len(flags) >= 20 and floor >= 2 and cap >= 1 and grew >= 3 and ls[4] == sum(flags)
    interval, lo, hi, s0, flags = R.LOSS_SCALE_RUNS[1]
    assert (interval, lo, hi) == (2000, 1.0, 2.0 ** 24)


# ---- fp32 arithmetic stays inside the bounds on the GPU module's inputs ----
@pytest.mark.parametrize("shape", [s for s, _ in R.MAXPOOL_ROWS], ids=str)
def test_fp32_restatement_of_maxpool_backward(shape):
    d = R.maxpool_inputs(shape)
    y = R.maxpool_fwd(d['x']).astype(np.float32)
    for act in R.ACTS:
        dx, M = R.maxpool_bwd(d['x'], y, d['dy'], act, A)
        dx32 = R.restate32_maxpool_bwd(d['x'], y, d['dy'], act, A)
        assert dx32.dtype == np.float32 and R.worst(dx32, dx, M) <= R.K_MAXPOOL_BWD[act], (act, R.worst(dx32, dx, M))
        if R.K_MAXPOOL_BWD[act] == 0:
            assert np.array_equal(dx32, dx)


@pytest.mark.parametrize("row", [r for r, _ in R.AVGPOOL_ROWS], ids=str)
def test_fp32_restatement_of_avgpool(row):
    shape, p = row
    x = Q.view_inputs(shape)['x']
    y, M = R.avgpool_fwd(x, p)
    y32 = R.restate32_avgpool_fwd(x, p)
    assert y32.dtype == np.float32 and R.worst(y32, y, M) <= R.k_avgpool_fwd(p) and R.rel(y32, y) <= R.REL_L2
    g = Q._rng(y.shape, 5).randn(*y.shape).astype(np.float32)
    dx, Md = R.avgpool_bwd(shape, g, p)
    assert R.worst(R.restate32_avgpool_bwd(shape, g, p), dx, Md) <= R.K_AVGPOOL_BWD


@pytest.mark.parametrize("row", [r for r, _ in R.UP_ROWS], ids=lambda r: "%s-%s" % (r[0], r[2]))
def test_fp32_restatement_of_the_resampling_kernels(row):
    d = R.up_inputs(row[0])
    lit, closed, M = R.bilinear_fwd(d['x'])
    y32 = R.restate32_bilinear_fwd(d['x'])
    assert y32.dtype == np.float32 and R.worst(y32, lit, M) <= R.K_BILINEAR_FWD and R.worst(y32, closed, M) <= R.K_BILINEAR_FWD
    dx, Md = R.bilinear_bwd(d['g'])
    dx32 = R.restate32_bilinear_bwd(d['g'])
    assert R.worst(dx32, dx, Md) <= R.K_BILINEAR_BWD and R.rel(dx32, dx) <= R.REL_L2, R.worst(dx32, dx, Md)
    nx, Mn = R.nearest_bwd(d['g'])
    assert R.worst(R.restate32_nearest_bwd(d['g']), nx, Mn) <= R.K_NEAREST_BWD
    assert R.bits_equal(R.nearest_fwd(d['x']), d['x'].repeat(2, 2).repeat(2, 3))


@pytest.mark.parametrize("kind", ['lsgan', 'bce'])
@pytest.mark.parametrize("n", [n for n, _ in R.LOSS_NS])
def test_fp32_restatement_of_the_scalar_losses(n, kind):
    d = R.loss_inputs(n, kind)
    for t in (0.0, 1.0):
        loss, Ml, g, Mg = R.scalar_loss(d, t, kind, 0.5)
        l32, g32 = R.restate32_scalar_loss(d, t, kind, 0.5)
        kl, kg = (R.K_LOSS, R.K_LSGAN_GRAD) if kind == 'lsgan' else (R.K_LIBM['bce_loss'], R.K_BCE_GRAD)
        assert abs(float(l32) - loss) <= kl * R.U * Ml, (abs(float(l32) - loss) / (R.U * Ml), kl)
        assert g32.dtype == np.float32 and R.worst(g32, g, Mg) <= kg and R.rel(g32, g) <= R.REL_L2, R.worst(g32, g, Mg)


@pytest.mark.parametrize("row", [r for r, _ in R.RECON_ROWS], ids=lambda r: "%s-%s-%s" % (r[0], r[1], r[3]))
def test_fp32_restatement_of_the_reconstruction_loss(row):
    shape, l2, va, vb, vg, gs = row
    d = R.recon_inputs(shape)
    loss, g, M = R.recon_loss(d['a'], d['b'], l2, gs)
    l32, g32 = R.restate32_recon_loss(d['a'], d['b'], l2, gs)
    assert abs(float(l32) - loss) <= R.K_LOSS * R.U * loss
    assert g32.dtype == np.float32 and R.worst(g32, g, M) <= R.K_RECON_GRAD and R.rel(g32, g) <= R.REL_L2


@pytest.mark.parametrize("n", [n for n, _ in R.OPT_NS])
def test_fp32_restatement_of_rmsprop_and_adam(n):
    d = R.opt_inputs(n)
    p2, Mp, a2, Ma = R.rmsprop(d['p'], d['g'], d['acc'], 1e-2, *R.RMSPROP_CONSTS, 0.5)
    p32, a32_ = R.restate32_rmsprop(d['p'], d['g'], d['acc'], 1e-2, *R.RMSPROP_CONSTS, 0.5)
    assert R.worst(a32_, a2, Ma) <= R.K_RMSPROP_ACC and R.worst(p32, p2, Mp) <= R.K_RMSPROP_P, (R.worst(a32_, a2, Ma), R.worst(p32, p2, Mp))
    for t0 in R.ADAM_T0:
        p3, Mp, m3, Mm, v3, Mv = R.adam(d['p'], d['g'], d['m'], d['acc'], t0, 1e-2, *R.ADAM_CONSTS, 0.5)
        p32, m32, v32 = R.restate32_adam(d['p'], d['g'], d['m'], d['acc'], t0, 1e-2, *R.ADAM_CONSTS, 0.5)
        assert R.worst(m32, m3, Mm) <= R.K_ADAM_M and R.worst(v32, v3, Mv) <= R.K_ADAM_V, (R.worst(m32, m3, Mm), R.worst(v32, v3, Mv))
        assert R.worst(p32, p3, Mp) <= R.K_LIBM['adam_p'], R.worst(p32, p3, Mp)


@pytest.mark.parametrize("row", [r for r, _ in R.IN_ROWS if np.prod(r[0]) <= 2 ** 18], ids=lambda r: "%s-g%d-%s" % (r[0], r[1], r[2]))
def test_fp32_restatement_of_the_instance_norm(row):
    shape, group, act, vx, vy, acc = row
    d = R.in_inputs(shape, group)
    y, M, mu, inv = R.instance_norm_fwd(d['x'], d['gamma'], d['beta'], act, A, group)
    y32 = R.restate32_instance_norm_fwd(d['x'], d['gamma'], d['beta'], act, A, group)
    k = R.K_LIBM['in_fwd_tanh'] if act == 'tanh' else R.K_IN_FWD[act]
    assert y32.dtype == np.float32 and R.worst(y32, y, M) <= k and R.rel(y32, y) <= R.REL_L2, R.worst(y32, y, M)
    if act == 'tanh':
        return
    m32, i32 = mu.astype(np.float32), inv.astype(np.float32)
    dx, Mx, dg, Mg, db, Mb = R.instance_norm_bwd(d['dout'], y32, d['x'], m32, i32, d['gamma'], act, A, group)
    xg, dg_, yg = (R.to_groups(v, group) for v in (d['x'], d['dout'], y32))
    dx32 = np.concatenate([Q.restate32_bn_backward(dg_[i:i + 1], yg[i:i + 1], xg[i:i + 1], m32[i], i32[i], d['gamma'], act, A)
                           for i in range(xg.shape[0])])
    assert R.worst(R.from_groups(dx32, group), dx, Mx) <= R.K_IN_BWD, R.worst(R.from_groups(dx32, group), dx, Mx)


def test_axpby_with_b_zero_is_one_product():
    x = Q.view_inputs((1, 1, 7, 9))['x']
    out = R.axpby_b0(0.3, x)
    assert out.dtype == np.float32 and R.worst(out, 0.3 * x.astype(np.float64), np.abs(0.3 * x)) <= 2
