"""CPU checks of tests/conv_s2_ref.py: the reference against torch in float64, the integer inputs' exactness claims, every
row's ``reaches`` claim through the library's host-only queries (under the row's own tuning environment), the table's
coverage, the calibration of k, and -- once -- that the per-element checks see what the whole-tensor norm does not."""
import ctypes as C

import numpy as np
import pytest

from gan_heightmaps_amd import device as D
from gan_heightmaps_amd._lib import call, load, tuning_env
from oracle import lp as LP
from tests import conv_s2_ref as R

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def desc(row):
    N, Cc, H, W, K = row.g
    xns, yns = R.strides(row)
    return D.conv_desc(N, Cc, H, W, K, 3, 3, 2, 1, xns, yns)


def variant(d, kind):
    out = C.create_string_buffer(128)
    call("ghm_conv2d_variant", C.byref(d), kind, out, 128)
    return out.value.decode()


def lp_variant(d, kind, mode):
    out = C.create_string_buffer(128)
    call("ghm_lp_variant", C.byref(d), kind, D.DTYPE_CODES[mode], out, 128)
    return out.value.decode()


# ---- the reference ----
@pytest.mark.parametrize("g", [(1, 12, 16, 64, 32), (3, 40, 12, 64, 32), (2, 16, 48, 32, 40)], ids=str)
def test_reference_agrees_with_torch_in_float64(g):
    torch = pytest.importorskip("torch")
    d = R.real_inputs(g)
    x = torch.tensor(d['x'].astype(np.float64), requires_grad=True)
    W = torch.tensor(d['W'].astype(np.float64), requires_grad=True)
    y = torch.nn.functional.conv2d(x, torch.flip(W, (2, 3)), torch.tensor(d['b'].astype(np.float64)), stride=2, padding=1)
    y.backward(torch.tensor(d['dy'].astype(np.float64)))
    for kind, want in (('fwd', y.detach().numpy()), ('dgrad', x.grad.numpy()), ('wgrad', W.grad.numpy())):
        got = R.ref(kind, d['x'], d['W'], d['b'] if kind == 'fwd' else None, d['dy'])
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), kind


@pytest.mark.parametrize("kind", R.KINDS)
def test_terms_are_the_reference_at_every_border_class(kind):
    """the explicit dot products that restate32 sums are the oracle's product, element by element (borders, corners, both
    parity classes), and sum |a| |b| is M"""
    g = (2, 12, 12, 64, 32)
    d = R.real_inputs(g)
    idx = R.sample_idx(kind, g, count=300)
    A, B, _ = R.operands(kind, d['x'], d['W'], d['dy'])
    a, b = R.terms(kind, A.astype(np.float64), B.astype(np.float64), idx)
    assert a.shape[1] == R.n_products(kind, g)
    ref, M = R.ref_mode('f32', kind, d['x'], d['W'], None, d['dy']), R.M('f32', kind, d['x'], d['W'], None, d['dy'])
    assert np.abs((a * b).sum(1) - R.at(ref, idx)).max() <= 1e-12 * M.max()
    assert np.abs(np.abs(a * b).sum(1) - R.at(M, idx)).max() <= 1e-12 * M.max()


def test_mode_references_are_the_oracles():
    """'bf16' / 'f16' and 'bf16x2' through this module == oracle/lp.py's statements (the definitions of the older tests)"""
    g = (1, 16, 8, 64, 32)
    d = R.real_inputs(g)
    for m in ('bf16', 'f16'):
        assert np.array_equal(R.ref_mode(m, 'fwd', d['x'], d['W'], d['b'], d['dy']), LP.conv2d_fwd(d['x'], d['W'], d['b'], 2, 1, m))
        dx, dW, _ = LP.conv2d_vjp(d['x'], d['W'], d['dy'], 2, 1, m)
        assert np.array_equal(R.ref_mode(m, 'dgrad', d['x'], d['W'], None, d['dy']), dx)
        assert np.array_equal(R.ref_mode(m, 'wgrad', d['x'], d['W'], None, d['dy']), dW)
    dx, dW = LP.conv2d_vjp_x2(d['x'], d['W'], d['dy'], 2, 1)
    scale = np.abs(dx).max()
    assert np.abs(R.ref_mode('bf16x2', 'fwd', d['x'], d['W'], d['b'], d['dy']) - LP.conv2d_fwd_x2(d['x'], d['W'], d['b'], 2, 1)).max() <= 1e-13 * scale
    assert np.abs(R.ref_mode('bf16x2', 'dgrad', d['x'], d['W'], None, d['dy']) - dx).max() <= 1e-13 * scale
    assert np.abs(R.ref_mode('bf16x2', 'wgrad', d['x'], d['W'], None, d['dy']) - dW).max() <= 1e-13 * np.abs(dW).max()


# ---- the integer inputs ----
@pytest.mark.parametrize("g", sorted({r.g for r in R.ROWS} | {q[2] for q in R.Q_ROWS}), ids=str)
def test_integer_inputs_are_exact_in_every_mode(g):
    d = R.int_inputs(g)
    for name in ('x', 'W', 'dy', 'b', 'bc'):
        a = d[name]
        assert np.array_equal(a, np.round(a)) and (a != 0).all(), name          # no zero anywhere, so none on a border
        assert np.array_equal(LP.round_bf16(a), a) and np.array_equal(LP.round_f16(a), a), name
        p = LP.split_bf16x3(a)
        assert not p[1].any() and not p[2].any(), name
    assert (d['yact'] == 0).any() and (d['yact'] > 0).any() and (d['yact'] < 0).any()
    for kind in R.KINDS:
        b = R.bias_of(kind, d)
        m = R.M('f32', kind, d['x'], d['W'], b, d['dy'], prev=d['prev'][kind])
        assert m.max() <= R.int_magnitude(kind, g), kind
        assert 2 * R.int_magnitude(kind, g) < 2 ** 24, kind                      # x 2: the accumulate form on top of itself
    # the results times the slope are exact too: quarter-integers below 2^22
    assert np.float32(R.SLOPE) == R.SLOPE and 4 * R.int_magnitude('wgrad', g) < 2 ** 24


# ---- the rows' claims ----
def reached(row):
    """what the library (host-only queries, planning with 256 CUs) and the restated planners say this row runs"""
    d, lib = desc(row), load()
    fam, kc = R.family(row.mode), R.KIND_CODE[row.kind]
    xns, yns = R.strides(row)
    if fam == 'f32':
        name, args, splits = R.parse_variant(variant(d, {'fwd': 0, 'dgrad': 3, 'wgrad': 2}[row.kind]))
        if row.kind == 'fwd':
            assert name == 'conv_patch_kernel' and args[0] == 3 and args[-1] == 2, name
            return dict(tile=(args[1], args[2]), splits=splits)
        if row.kind == 'dgrad':
            assert name == 'dgrad_s2_patch_kernel' and lib.ghm_dgrad_t_supported(C.byref(d)), name
            return dict(tile=(args[0], args[1]), splits=splits, dact=lib.ghm_dgrad_dact_supported(C.byref(d), 0))
        assert name == 'wgrad_patch_kernel' and args[:2] == [3, 2] and args[5] == 16, (name, args)
        return dict(bn=args[2], splits=splits)
    if fam == 'lp':
        dt = D.DTYPE_CODES[row.mode]
        assert lib.ghm_lp_supported(C.byref(d), kc, dt)
        want = {'fwd': 'lp_conv_kernel', 'dgrad': 'lp_dgrad_s2_kernel', 'wgrad': 'lp_wgrad_kernel'}[row.kind]
        assert lp_variant(d, kc, row.mode).startswith(want), lp_variant(d, kc, row.mode)      # not the small-map kernels
        assert row.kind == 'wgrad' or not R.small_map(row.g, row.kind)
        if row.kind == 'fwd':
            p = R.lp_plan(row.g, row.env)
            assert bool(lib.ghm_lp_q_direct(C.byref(d), 0, dt)) == (row.g[4] % 8 == 0 and (p['splits'] == 1 or p['finish'] == 'sm_finish'))
            out = dict(bm=p['bm'], tw=p['tw'], splits=p['splits'])
        elif row.kind == 'dgrad':
            p = R.lp_plan_dgrad_s2(row.g, row.env, xns)
            assert bool(lib.ghm_lp_q_direct(C.byref(d), 1, dt)) == (row.g[1] % 8 == 0 and p['splits'] == 1)
            out = dict(tile=(p['bm'], p['rt']), splits=p['splits'], dact=lib.ghm_dgrad_dact_supported(C.byref(d), dt))
            assert (out['dact'] == 3) == (p['splits'] == 1)
        else:
            p = R.lp_wplan(row.g, row.env, xns, yns)
            n = C.c_size_t()
            call("ghm_conv2d_wgrad_lp_workspace", C.byref(d), C.byref(n))
            assert n.value >= (p['splits'] * 9 * row.g[1] * row.g[4] * 4 if p['splits'] > 1 else 16)
            return dict(bn=p['bn'], nseg=p['nseg'], splits=p['splits'])
        if p['splits'] > 1:
            out['finish'] = p['finish']
        return out
    assert lib.ghm_split_supported(C.byref(d), kc)
    if row.kind == 'fwd':
        p = R.sp_plan(row.g, row.env)
        assert bool(lib.ghm_split_q_direct(C.byref(d), 0)) == (row.g[4] % 8 == 0 and p['splits'] == 1)
        return dict(tw=p['tw'], waves=p['waves'], splits=p['splits'], persistent=p['persistent'])
    if row.kind == 'dgrad':
        p = R.sp_plan_dgrad_s2(row.g, row.env, xns)
        assert bool(lib.ghm_split_q_direct(C.byref(d), 1)) == (row.g[1] % 8 == 0 and p['splits'] == 1)
        dact = 3 if lib.ghm_split_dgrad_dact_supported(C.byref(d)) else 0
        assert (dact == 3) == (p['splits'] == 1)
        return dict(splits=p['splits'], dact=dact)
    p = R.sp_wplan(row.g, row.env)
    n = C.c_size_t()
    call("ghm_conv2d_wgrad_split_workspace", C.byref(d), C.byref(n))
    assert n.value == p['splits'] * 9 * row.g[1] * row.g[4] * 4            # the library's own split count
    return dict(spx=p['spx'], splits=p['splits'])


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row_reaches_what_it_claims(row):
    assert row.view in R.VIEWS and max(np.prod(s) for s in R.shapes(row.g)) <= 2 ** 19 + 2 ** 17
    with tuning_env(**row.env):
        got = reached(row)
    assert got == row.reaches, (got, row.reaches)


def _cover(row):
    r, fam = row.reaches, R.family(row.mode)
    if fam == 'f32' or (fam == 'lp' and row.kind == 'dgrad'):
        tile = r['tile'] if row.kind != 'wgrad' else r['bn']
    elif fam == 'lp':
        tile = (r['bm'], r['tw']) if row.kind == 'fwd' else (r['bn'], r['nseg'])
    elif row.kind == 'fwd':
        tile = (r['tw'], r['waves'], r['persistent'])
    else:
        tile = (64, 2) if row.kind == 'dgrad' else r['spx']
    return fam, row.kind, tile, r['splits'] > 1


def test_table_covers_every_tile_and_split_path():
    for modes in (('f32',), ('bf16',), ('f16',), ('bf16x3',), ('bf16x2',)):
        rows = [r for r in R.ROWS if r.mode in modes]
        have = {_cover(r) for r in rows}
        want = {c for c in R.COVERAGE if c[0] == R.family(modes[0])}
        assert want <= have, sorted(want - have, key=str)
        for kind in R.KINDS:                    # every view spec per kind and mode; both finishing kernels of the lp split-K
            assert {r.view for r in rows if r.kind == kind} == set(R.VIEWS), (modes, kind)
        if R.family(modes[0]) == 'lp':
            assert {r.reaches.get('finish') for r in rows} >= {'sm_finish', 'splitk_finish'}
        assert any(r.kind == 'dgrad' and r.reaches['dact'] for r in rows)
    # a forced split count that does not divide the slab count, in every family and kind that takes one
    ragged = [('f32', 'fwd', 9, 2), ('f32', 'dgrad', 9, 2), ('f32', 'wgrad', 50, 3), ('lp', 'fwd', 3, 2), ('lp', 'dgrad', 3, 2),
              ('lp', 'wgrad', 24, 5), ('split', 'fwd', 5, 2)]
    for fam, kind, slabs, splits in ragged:
        assert slabs % splits and any(R.family(r.mode) == fam and r.kind == kind and r.reaches['splits'] == splits and _slabs(r) == slabs
                                      for r in R.ROWS), (fam, kind)
    assert len({(m, k) for m, k, _, _ in R.Q_ROWS}) == len(R.Q_ROWS) == 8


def _slabs(r):
    N, Cc, H, W, K = r.g
    fam = R.family(r.mode)
    if r.kind == 'wgrad':
        return N * (H // 2) * (W // 2) // 16 if fam == 'f32' else (R.lp_wplan(r.g, r.env)['slabs'] if fam == 'lp' else 0)
    red = Cc if r.kind == 'fwd' else K
    return red // (4 if fam == 'f32' else 16)


@pytest.mark.parametrize("q", R.Q_ROWS, ids=lambda q: "%s-%s" % q[:2])
def test_q_rows_are_single_pass(q):
    mode, kind, g, view = q
    N, Cc, H, W, K = g
    d, lib = D.conv_desc(N, Cc, H, W, K, 3, 3, 2, 1), load()
    if mode in D.SPLITS:
        assert lib.ghm_split_q_direct(C.byref(d), R.KIND_CODE[kind])
    else:
        assert lib.ghm_lp_q_direct(C.byref(d), R.KIND_CODE[kind], D.DTYPE_CODES[mode])
        assert lp_variant(d, R.KIND_CODE[kind], mode).startswith('lp_conv_kernel' if kind == 'fwd' else 'lp_dgrad_s2_kernel')
        assert (R.lp_plan(g, {}) if kind == 'fwd' else R.lp_plan_dgrad_s2(g, {}))['splits'] == 1


# ---- k ----
def measure(mode, kind):
    worst_k = 0.0
    for g in sorted({r.g for r in R.ROWS if r.mode == mode and r.kind == kind}):
        def one():
            d = R.real_inputs(g)
            b, idx = R.bias_of(kind, d), R.sample_idx(kind, g)
            ref = R.at(R.ref_mode(mode, kind, d['x'], d['W'], b, d['dy']), idx)
            m = R.at(R.M(mode, kind, d['x'], d['W'], b, d['dy']), idx)
            return R.worst(R.restate32(kind, mode, d['x'], d['W'], b, d['dy'], idx), ref, m)
        worst_k = max(worst_k, cached(('k', mode, kind, g), one))
    return worst_k


@pytest.mark.parametrize("mode", R.MODES)
def test_k_is_twice_the_sequential_fp32_restatement(mode):
    for kind in R.KINDS:
        w = measure(mode, kind)
        k = R.K_BOUND[(mode, kind)]
        print("%s %s: restate32 worst %.2f x 2^-24 M -> k = %d (frozen %d)" % (mode, kind, w, int(np.ceil(2 * w)), k))
        assert k == int(np.ceil(2 * w)), (mode, kind, w, k)
        for r in R.ROWS:
            if r.mode == mode and r.kind == kind:
                assert k <= R.n_products(kind, r.g) + r.reaches['splits'] + 2, r


# ---- sensitivity ----
def test_per_element_checks_see_what_the_norm_does_not():
    """(a) one first-order correction product (x1 w0 of one tap, of typical size) missing at one border element of a 'bf16x3' forward: inside
    the rel-L2 bound, far outside k; (b) the last row of a data gradient computed with the other parity class's tap row: the
    integer pass sees every element of it (the norm sees this one too: a whole wrong row of integers is not small)"""
    g, mode = (3, 32, 32, 128, 48), 'bf16x3'
    d = R.real_inputs(g)
    ref, m = R.ref_mode(mode, 'fwd', d['x'], d['W'], d['b'], d['dy']), R.M(mode, 'fwd', d['x'], d['W'], d['b'], d['dy'])
    good = ref.astype(np.float32)
    assert R.worst(good, ref, m) <= 1 and R.rel(good, ref) < R.REL_L2[mode]
    idx = np.array([[2, 5, 15, 63]])                             # last output row and column: a tile's edge
    a, b = R.terms('fwd', R.pieces(d['x'], mode)[1], R.pieces(d['W'], mode)[0], idx)
    units = np.abs(a[0] * b[0]) / (R.U * R.at(m, idx)[0])
    print("first-order correction products at the element: %d of %d above k, median %.1f, largest %.1f x 2^-24 M"
          % ((units > R.K_BOUND[(mode, 'fwd')]).sum(), units.size, np.median(units), units.max()))
    t = int(np.argmin(np.abs(units - 100)))                      # a typical one of those a dropped tap row loses: 100 units
    bad = ref.copy()
    bad[tuple(idx[0])] -= float(a[0, t]) * float(b[0, t])
    bad = bad.astype(np.float32)
    w, r = R.worst(bad, ref, m), R.rel(bad, ref)
    print("dropped correction product: %.1f x 2^-24 M at the element (k = %d), rel-L2 %.2e (bound %.0e)" % (w, R.K_BOUND[(mode, 'fwd')], r, R.REL_L2[mode]))
    assert w > R.K_BOUND[(mode, 'fwd')] and r < R.REL_L2[mode]
    di = R.int_inputs(g)
    iref = R.ref('dgrad', None, di['W'], None, di['dy'])
    swapped = iref.copy()
    dyp = np.concatenate([di['dy'][:, :, 1:], di['dy'][:, :, :1]], axis=2)       # the last row's taps from the other class row
    swapped[:, :, -1] = R.ref('dgrad', None, di['W'], None, dyp)[:, :, -1]
    differ = (swapped != iref)[:, :, -1].mean()
    print("swapped parity class of the last row: %.0f %% of its elements differ in bits, rel-L2 %.2e" % (100 * differ, R.rel(swapped, iref)))
    assert differ > 0.9 and not (swapped != iref)[:, :, :-1].any()
