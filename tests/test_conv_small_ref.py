"""CPU checks of tests/conv_small_ref.py: the reference against torch in float64 at every (filter, stride, padding) used, the
explicit terms at every border class, the integer inputs' exactness claims, every row's ``reaches`` claim through the restated
planner AND the library's host-only ghm_sm_plan_query (under the row's own tuning environment), the table's coverage, the
calibration of every k, the LDS limit of the ring, and -- once -- that the per-element check sees what the whole-tensor norm
does not."""
import ctypes as C

import numpy as np
import pytest

from gan_heightmaps_amd import device as D
from gan_heightmaps_amd._lib import call, load, tuning_env
from oracle import lp as LP
from tests import conv_small_ref as R

_CACHE = {}
GEOMS = sorted({r.g for r in R.ROWS})


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def desc(g):
    N, Cc, H, W, K, k, s, pad = g
    return D.conv_desc(N, Cc, H, W, K, k, k, s, pad)


def query(g, kind, mode):
    """ghm_sm_plan_query -> the planner's dict (None: not served)"""
    out = (C.c_int32 * 12)()
    call("ghm_sm_plan_query", C.byref(desc(g)), R.KIND_CODE[kind], D.DTYPE_CODES[mode], C.byref(out))
    q = list(out)
    if not q[0]:
        assert not any(q)
        return None
    return dict(ncls=q[1], ntaps=q[2], nq=q[3], nimg=q[4], rows=q[5], splits=q[6], sps=q[7], pfs=q[8], lds=q[9], finish=q[10],
                cls=tuple((q[11] >> (8 * c)) & 255 for c in range(q[1])))


# ---- the reference ----
def _one_per_filter():
    seen = {}
    for r in R.ROWS:
        seen.setdefault(r.g[5:], r.g)
        if r.g[2] != r.g[3]:
            seen[r.g[5:] + ('non-square',)] = r.g
    return sorted(seen.values())


@pytest.mark.parametrize("g", _one_per_filter(), ids=str)
def test_reference_agrees_with_torch_in_float64(g):
    torch = pytest.importorskip("torch")
    N, Cc, H, W, K, k, s, pad = g
    d = R.real_inputs(g)
    x = torch.tensor(d['x'].astype(np.float64), requires_grad=True)
    Wt = torch.tensor(d['W'].astype(np.float64))
    y = torch.nn.functional.conv2d(x, torch.flip(Wt, (2, 3)), torch.tensor(d['b'].astype(np.float64)), stride=s, padding=pad)
    y.backward(torch.tensor(d['dy'].astype(np.float64)))
    for kind, want in (('fwd', y.detach().numpy()), ('dgrad', x.grad.numpy())):
        got = R.ref(kind, g, d['x'], d['W'], d['b'] if kind == 'fwd' else None, d['dy'])
        assert got.dtype == np.float64 and got.shape == want.shape == R.out_shape(kind, g)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), kind


@pytest.mark.parametrize("g", _one_per_filter(), ids=str)
def test_terms_are_the_reference_at_every_border_class(g):
    """the explicit dot products that restate32 sums are the oracle's product, element by element (borders, corners, the four
    parity classes), sum |a| |b| is M, and the sample holds every border and parity class"""
    d = R.real_inputs(g)
    for kind in R.KINDS:
        idx = R.sample_idx(kind, g, count=200)
        shp = R.out_shape(kind, g)
        for ax in (2, 3):
            assert {0, shp[ax] - 1} <= set(idx[:, ax])
        if kind == 'dgrad' and g[6] == 2:
            assert {(i % 2, j % 2) for i, j in idx[:, 2:]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            assert sum(R.class_taps(g)) == g[5] ** 2
        A = d['x'] if kind == 'fwd' else d['dy']
        a, b = R.terms(kind, g, A.astype(np.float64), d['W'].astype(np.float64), idx)
        assert a.shape[1] == R.n_products(kind, g)
        ref, M = R.ref(kind, g, d['x'], d['W'], None, d['dy']), R.ref(kind, g, np.abs(d['x']), np.abs(d['W']), None, np.abs(d['dy']))
        assert np.abs((a * b).sum(1) - R.at(ref, idx)).max() <= 1e-12 * M.max(), kind
        assert np.abs(np.abs(a * b).sum(1) - R.at(M, idx)).max() <= 1e-12 * M.max(), kind


def test_mode_references_are_the_oracles():
    g = (3, 16, 8, 8, 16, 5, 2, 2)
    d = R.real_inputs(g)
    for m in R.MODES:
        assert np.array_equal(R.ref_mode(m, 'fwd', g, d['x'], d['W'], d['b'], None), LP.conv2d_fwd(d['x'], d['W'], d['b'], 2, 2, m))
        assert np.array_equal(R.ref_mode(m, 'dgrad', g, None, d['W'], None, d['dy']), LP.conv2d_vjp(d['x'], d['W'], d['dy'], 2, 2, m)[0])


# ---- the integer inputs ----
@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_integer_inputs_are_exact_in_both_modes(g):
    d = R.int_inputs(g)
    for name in ('x', 'W', 'dy', 'b', 'bc'):
        a = d[name]
        assert np.array_equal(a, np.round(a)) and (a != 0).all(), name          # no zero anywhere, so none on a border
        assert np.array_equal(LP.round_bf16(a), a) and np.array_equal(LP.round_f16(a), a), name
    for kind in R.KINDS:
        m = R.M('bf16', kind, g, d['x'], d['W'], R.bias_of(kind, d), d['dy'], prev=d['prev'][kind])
        assert m.max() <= R.int_magnitude(kind, g), kind
        assert 2 * R.int_magnitude(kind, g) < 2 ** 24, kind                      # any summation order is exact
        assert 4 * R.int_magnitude(kind, g) < 2 ** 24                            # ... and so is the result times the slope
    assert np.float32(R.SLOPE) == R.SLOPE


# ---- the rows' claims ----
@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row_reaches_what_it_claims(row):
    assert row.view in R.VIEWS
    p = R.sm_plan(row.g, row.kind, row.env)
    assert p is not None and R.claim(p) == row.reaches, (p, row.reaches)
    with tuning_env(**row.env):
        q = query(row.g, row.kind, row.mode)
        name = C.create_string_buffer(128)
        call("ghm_lp_variant", C.byref(desc(row.g)), R.KIND_CODE[row.kind], D.DTYPE_CODES[row.mode], name, 128)
        assert load().ghm_lp_q_direct(C.byref(desc(row.g)), R.KIND_CODE[row.kind], D.DTYPE_CODES[row.mode])
    assert name.value.decode().startswith("sm_gemm_kernel<"), name.value
    assert q == {f: p[f] for f in q}, (q, p)
    assert p['lds'] <= R.MAX_LDS and 3 <= p['pfs'] <= R.ring(p['ntaps'], p['nq'])[2]
    assert (p['pfs'] - 2) * R.ring(p['ntaps'], p['nq'])[1] <= 60           # the 6-bit vmcnt of the ring's wait


def test_unserved_geometries_are_reported_as_such():
    for g, kind in (((5, 16, 4, 4, 24, 1, 1, 0), 'dgrad'), ((2, 16, 32, 32, 16, 5, 2, 2), 'fwd'), ((2, 16, 6, 6, 16, 3, 1, 1), 'fwd'),
                    ((3, 16, 16, 16, 16, 3, 1, 1), 'fwd')):
        assert R.sm_plan(g, kind, {}) is None and query(g, kind, 'bf16') is None, (g, kind)
    assert query((2, 16, 4, 4, 16, 3, 1, 1), 'fwd', 'f32') is None


@pytest.mark.parametrize("row", R.BN_ROWS, ids=R.bn_row_id)
def test_batchnorm_row_reaches_what_it_claims(row):
    form, pixels, splits = row.reaches
    N, Cc, H, W, K, k, s, pad = row.g
    Ho, Wo = R.out_hw(row.g)
    assert pixels == N * Ho * Wo and form == (256 if pixels <= 256 else 1024) and K % 8 == 0 and K > R.ZERO_CHANNEL
    lib, d = load(), desc(row.g)
    with tuning_env(**row.env):
        for mode in R.MODES:
            q = query(row.g, 'fwd', mode)
            if row.path == 'sm':
                p = R.sm_plan(row.g, 'fwd', row.env)
                assert q is not None and q == {f: p[f] for f in q} and (q['finish'], p['pixels'], q['splits']) == row.reaches
                assert lib.ghm_conv_bn_fused_supported(C.byref(d), D.DTYPE_CODES[mode])
            elif row.path == 'splitk':
                assert q is None and lib.ghm_conv_bn_fused_supported(C.byref(d), D.DTYPE_CODES[mode])
                assert R.lp_splits(row.g, row.env) == splits
        if row.path == 'f32':
            assert lib.ghm_conv_bn_fused_supported_f32(C.byref(d))


def test_table_covers_the_family():
    for mode in R.MODES:
        rows = [r for r in R.ROWS if r.mode == mode]
        plans = [(r, R.sm_plan(r.g, r.kind, r.env)) for r in rows]
        assert {(p['ntaps'], p['nq']) for _, p in plans} == {(t, q) for t in (4, 9, 25) for q in (1, 2, 5)}
        for depth in (3, 4, 5, 6, 7, 8):            # every ring depth, each with a block that goes round the ring twice or more
            assert any(p['pfs'] == depth and p['sps'] >= 2 * depth + 1 and p['splits'] == 1 for _, p in plans), depth
        assert any(p['sps'] == 32 for _, p in plans)
        assert any(p['splits'] > 8 for _, p in plans)
        assert any(p['splits'] > 1 and p['last'] != p['sps'] for _, p in plans)                  # a ragged last split
        assert {p['cls'] for _, p in plans if p['ncls'] == 4} >= {(1, 2, 2, 4), (4, 4, 4, 4), (9, 6, 6, 4), (1, 1, 1, 1)}
        assert any(p['pixels'] < 256 for _, p in plans) and any(p['pixels'] > 256 and p['pixels'] % 256 == 0 for _, p in plans)
        assert any(p['nimg'] > 1 and r.g[0] % p['nimg'] for r, p in plans)                       # an image group that is not full
        assert any(p['nimg'] == 1 for _, p in plans)
        assert {r.g[5] for r in rows} == {1, 2, 3, 4, 5} and any(r.g[2] != r.g[3] for r in rows)
        assert {r.g[4] if r.kind == 'fwd' else r.g[1] for r in rows} >= {8, 16, 24, 40}          # row tiles: quarter, half, ragged
        for kind in R.KINDS:
            assert {r.view for r in rows if r.kind == kind} == set(R.VIEWS), kind
    forms = {(r.reaches[0], r.reaches[1] in (256, 1024)) for r in R.BN_ROWS}
    assert forms == {(256, True), (256, False), (1024, True), (1024, False)}                      # both forms, full and ragged
    assert {r.reaches[1] for r in R.BN_ROWS} >= {2, 20, 48, 192, 256, 320, 768, 1024}
    assert {r.path for r in R.BN_ROWS} == {'sm', 'splitk', 'f32'}
    assert any(r.reaches[2] > 8 for r in R.BN_ROWS) and any(r.path == 'sm' and r.reaches[2] > 1 for r in R.BN_ROWS)


# ---- the LDS limit of the ring ----
def test_a_ring_budget_above_the_lds_is_clamped_to_it():
    """GHM_SM_LDS_KB is a wish for depth: above 160 KB it plans what 160 KB plans (launched by no test)"""
    g, kind = (3, 64, 16, 4, 16, 5, 1, 2), 'fwd'            # (25, 5): 48 KB slots, up to 7 of them
    with tuning_env(GHM_SM_SPLITS='1', GHM_SM_LDS_KB='160'):
        at160 = query(g, kind, 'bf16')
    assert (at160['ntaps'], at160['nq'], at160['sps'], at160['pfs'], at160['lds']) == (25, 5, 4, 3, 3 * 49152)
    for kb in (161, 240, 400, 100000):
        with tuning_env(GHM_SM_SPLITS='1', GHM_SM_LDS_KB=str(kb)):
            q = query(g, kind, 'bf16')
        assert q == at160 and q['lds'] <= R.MAX_LDS, (kb, q)
        assert R.claim(R.sm_plan(g, kind, {'GHM_SM_SPLITS': '1', 'GHM_SM_LDS_KB': str(kb)}))[-1] == 3
    for t in (4, 9, 25):                                     # three slots, the minimum, fit for every variant
        for nq in (1, 2, 5):
            assert 3 * R.ring(t, nq)[0] * 16 <= R.MAX_LDS


# ---- k ----
def measure(mode, kind):
    worst_k = 0.0
    geoms = {r.g for r in R.ROWS if r.mode == mode and r.kind == kind} if mode != 'f32' else {r.g for r in R.BN_ROWS if r.path == 'f32'}
    for g in sorted(geoms):
        def one():
            d = R.real_inputs(g)
            b, idx = R.bias_of(kind, d), R.sample_idx(kind, g)
            ref = R.at(R.ref_mode(mode, kind, g, d['x'], d['W'], b, d['dy']), idx)
            m = R.at(R.M(mode, kind, g, d['x'], d['W'], b, d['dy']), idx)
            return R.worst(R.restate32(kind, mode, g, d['x'], d['W'], b, d['dy'], idx), ref, m)
        worst_k = max(worst_k, cached(('k', mode, kind, g), one))
    return worst_k


@pytest.mark.parametrize("mode", R.MODES + ('f32',))
def test_k_is_twice_the_sequential_fp32_restatement(mode):
    for kind in (R.KINDS if mode != 'f32' else ('fwd',)):
        w = measure(mode, kind)
        k = R.K_BOUND[(mode, kind)]
        print("%s %s: restate32 worst %.2f x 2^-24 M -> k = %d (frozen %d)" % (mode, kind, w, int(np.ceil(2 * w)), k))
        assert k == int(np.ceil(2 * w)), (mode, kind, w, k)
        for r in R.ROWS:
            if r.mode == mode and r.kind == kind:
                assert k <= R.n_products(kind, r.g) + r.reaches[5] + 2, r
        for r in R.BN_ROWS:                     # their conv_out is held to the forward k of its arithmetic
            if kind == 'fwd' and (mode == 'f32') == (r.path == 'f32'):
                assert k <= R.n_products('fwd', r.g) + max(r.reaches[2], 1) + 2, r


def test_batchnorm_bounds_are_twice_the_fp32_restatement():
    w = dict(y=0.0, mean=0.0, inv=0.0, run=0.0)
    for row in R.BN_ROWS:
        for mode in (R.MODES if row.path != 'f32' else ('f32',)):
            d = R.bn_inputs(row.g)
            r = LP.ROUND[mode]
            t = R.ref('fwd', row.g, r(d['x']), r(d['W']), d['b'], None).astype(np.float32)
            assert np.array_equal(t[:, R.ZERO_CHANNEL], np.full_like(t[:, 0], d['b'][R.ZERO_CHANNEL]))
            for act in ('lrelu', 'linear'):
                ref, got = R.bn_ref(t, d, act, R.BN_SLOPE), R.restate32_bn(t, d, act, R.BN_SLOPE)
                w['y'] = max(w['y'], R.worst(got['y'], ref['y'], ref['M']))
            w['mean'] = max(w['mean'], R.worst(got['mean'], ref['mean'], ref['M_mean']))
            w['inv'] = max(w['inv'], R.worst(got['inv'], ref['inv'], ref['inv']))
            w['run'] = max(w['run'], R.worst(got['rm'], ref['rm'], ref['M_rm']), R.worst(got['ri'], ref['ri'], ref['M_ri']))
            # the all-zero filter: mean == bias, inv == fl32(1 / sqrt(eps)), y == act(beta), bit for bit
            z = R.ZERO_CHANNEL
            assert got['mean'][z] == d['b'][z] and got['inv'][z] == np.float32(1.0 / np.sqrt(float(np.float32(R.BN_EPS))))
            assert np.array_equal(got['y'][:, z], np.full_like(t[:, z], d['beta'][z]))
    print("restate32_bn worst: y %.2f  mean %.2f  inv %.2f  running %.2f" % (w['y'], w['mean'], w['inv'], w['run']))
    for name, k in (('y', R.K_BN), ('mean', R.K_MEAN), ('inv', R.K_INV), ('run', R.K_RUN)):
        assert k == int(np.ceil(2 * w[name])), (name, w[name], k)


# ---- sensitivity ----
def test_per_element_check_sees_a_wrong_border_element_that_the_norm_does_not():
    """one product of typical size missing at one corner element of a 4 x 4 map: far inside the rel-L2 bound of
    tests/test_gpu_lp.py, far outside k"""
    g, mode, kind = (5, 32, 4, 4, 16, 3, 1, 1), 'bf16', 'fwd'
    assert any(r.g == g and r.kind == kind for r in R.ROWS)
    d = R.real_inputs(g)
    ref, m = R.ref_mode(mode, kind, g, d['x'], d['W'], d['b'], None), R.M(mode, kind, g, d['x'], d['W'], d['b'], None)
    good = ref.astype(np.float32)
    assert R.worst(good, ref, m) <= 1 and R.rel(good, ref) < R.REL_L2[mode]
    idx = np.array([[4, 15, 3, 3]])                              # last image, last filter, the corner: four of nine taps are padding
    a, b = R.terms(kind, g, LP.ROUND[mode](d['x']), LP.ROUND[mode](d['W']), idx)
    assert (a[0] == 0).sum() == 5 * g[1]
    units = np.abs(a[0].astype(np.float64) * b[0]) / (R.U * R.at(m, idx)[0])
    t = int(np.argmin(np.abs(units - 100)))
    bad = ref.copy()
    bad[tuple(idx[0])] -= float(a[0, t]) * float(b[0, t])
    bad = bad.astype(np.float32)
    w, r = R.worst(bad, ref, m), R.rel(bad, ref)
    print("one dropped product: %.1f x 2^-24 M at the element (k = %d), rel-L2 %.2e (bound %.0e)" % (w, R.K_BOUND[(mode, kind)], r, R.REL_L2[mode]))
    assert w > R.K_BOUND[(mode, kind)] and r < R.REL_L2[mode] and (bad != good).sum() == 1


def test_integer_pass_sees_a_wrong_class_a_stale_slab_and_a_wrapped_border():
    """three ways this family can go wrong, applied to the reference: every element they touch differs in bits in the integer
    pass, and nothing else does"""
    from oracle import ops as O
    # (a) one parity class of a 5x5 stride-2 data gradient walks a tap too few (class 1: 6 taps)
    g = (3, 16, 8, 8, 16, 5, 2, 2)
    d = R.int_inputs(g)
    ref = R.ref('dgrad', g, None, d['W'], None, d['dy'])
    W1 = d['W'].copy()
    W1[:, :, 0, 1] = 0                      # a tap that only the classes of odd columns and even rows read
    mut = ref.copy()
    mut[:, :, 0::2, 1::2] = R.ref('dgrad', g, None, W1, None, d['dy'])[:, :, 0::2, 1::2]
    hit = mut != ref
    print("(a) dropped tap of parity class 1: %.0f %% of its elements differ" % (100 * hit[:, :, 0::2, 1::2].mean()))
    assert hit[:, :, 0::2, 1::2].mean() > 0.5 and hit.sum() == hit[:, :, 0::2, 1::2].sum()
    # (b) a ring slot read before its DMA landed: slab 4 of 7 holds slab 1's bytes for the first wave's 32 pixels
    g = (3, 112, 4, 4, 16, 3, 1, 1)
    d = R.int_inputs(g)
    ref = R.ref('fwd', g, d['x'], d['W'], None, None)

    def slab(s):
        x = np.zeros_like(d['x'])
        x[:, 16 * s:16 * s + 16] = d['x'][:, 16 * s:16 * s + 16]
        return x
    stale = np.zeros_like(d['x'])
    stale[:, 64:80] = d['x'][:, 16:32]      # slab 1's window under slab 4's weights
    mut = ref.copy()
    mut[:2] += (R.ref('fwd', g, stale, d['W'], None, None) - R.ref('fwd', g, slab(4), d['W'], None, None))[:2]
    hit = mut != ref
    print("(b) stale ring slot: %.0f %% of the wave's elements differ" % (100 * hit[:2].mean()))
    assert hit[:2].mean() > 0.9 and not hit[2:].any()
    # (c) the left border of a non-square map reads data where the padding is
    g = (3, 16, 4, 8, 16, 3, 1, 1)
    d = R.int_inputs(g)
    ref = R.ref('fwd', g, d['x'], d['W'], None, None)
    xw = np.pad(d['x'].astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)), mode='wrap')
    xw[:, :, 0] = xw[:, :, -1] = 0
    mut = ref.copy()
    mut[:, :, :, 0] = O.conv2d_fwd(xw, d['W'].astype(np.float64), np.zeros(16), 1, 0)[:, :, :, 0]
    hit = mut != ref
    print("(c) wrapped left border: %.0f %% of the column's elements differ" % (100 * hit[:, :, :, 0].mean()))
    assert hit[:, :, :, 0].mean() > 0.9 and not hit[:, :, :, 1:].any()
