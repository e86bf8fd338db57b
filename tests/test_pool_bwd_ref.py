"""CPU checks of tests/pool_bwd_ref.py: the definition against oracle.ops on the full path conv -> activation -> max-pool,
its tie semantics against elementwise_q_ref.mask_bwd, the compressed form against the dense one, the masks' inventory, the
integer inputs' exactness condition, every row's ``reaches`` claim through the library's host-only queries, the calibration
of k, and -- by mutating the numpy reference, never a kernel -- what the per-element check sees and what the older tests'
rel-L2 <= 1e-5 says of the same mutation (MUTATIONS records both).  At the older test's geometry (3, 96, 128, 64) the norm
fails on the issue's five as well (the closest: a column bit flipped in ONE window moves dW by 3.5e-05); the same flip in a
window whose gradient is 4e-3 of the tensor's rms passes it (7.2e-06, 7.9e-06) while the per-element check stands 78 (dW)
and 1487 (dx) units of 2^-24 M over.  The norm also cannot say where, and is only ever taken at five large shapes in lrelu.
Wall time without a GPU: 69 tests in 3.4 s.
"""
import ctypes as C
import math

import numpy as np
import pytest

from gan_heightmaps_amd import device as D
from gan_heightmaps_amd._lib import call, load, tuning_env
from oracle import ops as O
from tests import elementwise_q_ref as Q
from tests import pool_bwd_ref as R

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def desc(g, view='whole', xns=None):
    N, H, W, K = g
    return D.conv_desc(N, 1, H, W, K, 5, 5, 1, 2, R.view_layout((N, 1, H, W), view)[1] if xns is None else xns)


def split_desc(g):
    N, Cc, K, H, W = g
    return D.conv_desc(N, Cc, H, W, K, 5, 5, 1, 2)


def supported(d, act='lrelu'):
    return int(load().ghm_conv2d_pool_bwd_sparse_supported(C.byref(d), D.ACT_CODES[act]))


def ws_bytes(name, d):
    n = C.c_size_t()
    call(name, C.byref(d), C.byref(n))
    return n.value


# ---- the definition ----
@pytest.mark.parametrize("g", [(2, 8, 12, 3), (3, 6, 10, 5)], ids=str)
def test_reference_is_the_oracle_vjp_of_conv_activation_maxpool(g):
    N, H, W, K = g
    d = R.inputs(g, ((), ()), False)
    x = d['x'].astype(np.float64)
    x[:, :, :H // 2, :W // 2] = 0.25            # constant patch: tied windows
    x[-1] = 0.0
    Wt, b, gp = d['W'].astype(np.float64), d['prev_db'].astype(np.float64), d['gp'].astype(np.float64)
    z = O.conv2d_fwd(x, Wt, b, 1, 2)
    for act in ('lrelu', 'relu', 'linear'):
        a = {'lrelu': O.lrelu_fwd(z, R.SLOPE), 'relu': O.relu_fwd(z), 'linear': z}[act]
        p = O.maxpool_fwd(a)
        da = O.maxpool_vjp(a, p, gp)
        dz = {'lrelu': lambda: O.lrelu_vjp(z, R.SLOPE, da), 'relu': lambda: O.relu_vjp(z, da), 'linear': lambda: da}[act]()
        dx, dW, db = O.conv2d_vjp(x, Wt, dz, 1, 2)
        _, mask = R.pool_ref(a)
        assert ((mask & 15) == 15).any() and (np.unpackbits((mask & 15)[..., None], axis=-1).sum(-1) == 1).any()
        for yp in (p, None):
            got = R.ref(x, Wt, mask, yp, gp, act, R.SLOPE)
            for name, want in (('dW', dW), ('db', db), ('dx', dx)):
                assert np.abs(got[name] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-30), (act, name, yp is None)


def test_tie_semantics_are_mask_bwd_and_the_compressed_form_is_the_dense_one():
    d = Q.pool_inputs((3, 24, 20, 64))
    for act in R.ACTS:
        for y in (d['y'], None):
            want = Q.mask_bwd(d['mask'], y, d['dy'], act, R.ALPHA)[0]
            assert np.array_equal(R.dense_grad(d['mask'], y, d['dy'], act, R.ALPHA), want)
    ev = d['mask'][:, :, ::2]                                              # every other pooled row: no tied window row
    ev[(ev & 3) == 3] &= 0xfd
    ev[(ev & 12) == 12] &= 0xf7
    G32 = R.dense_grad(d['mask'], d['y'], d['dy'], 'lrelu', R.ALPHA, np.float32)
    cq, idx, flags = R.compressed(d['mask'], d['y'], d['dy'], 'lrelu', R.ALPHA, 'bf16x3')
    N, K, Hp, Wp = d['mask'].shape
    val = sum(c.astype(np.float64) for c in cq).astype(np.float32)                        # the pieces add up to the value exactly
    col = ((idx.transpose(0, 1, 4, 2, 3)[..., None] >> np.arange(16)) & 1).reshape(N, K, 2 * Hp, Wp)
    fl = flags.reshape(N, 2 * Hp).astype(bool)
    # a row without a flag expands to the dense row; in a flagged row the tied windows hold v in both columns
    ex = np.zeros_like(G32)
    ex[..., 0::2] = np.where(col == 0, val, 0)
    ex[..., 1::2] = np.where(col == 1, val, 0)
    free = ~fl[:, None, :, None] & np.ones(G32.shape, bool)
    assert np.array_equal(ex[free], G32[free]) and fl.any() and not fl.all()
    tied = (G32[..., 0::2] != 0) & (G32[..., 1::2] != 0)
    assert np.array_equal(tied.any(axis=(1, 3)), fl)                  # (leaky slope: v is never zero)
    assert np.array_equal(np.where(tied, val, 0), np.where(tied, G32[..., 0::2], 0))
    assert idx.dtype == np.uint16 and idx.shape == (N, K // 8, 2 * Hp, Wp // 16, 8) and flags.dtype == np.int32


# ---- the inputs ----
def inventory(mask, yp, seams):
    nib = mask & 15
    N, K, Hp, Wp = nib.shape
    assert np.array_equal((mask & 16) != 0, yp > 0) and (mask < 32).all()
    if nib.size >= 256 and max(Hp, Wp) >= 16:
        assert set(np.unique(np.unpackbits(nib[..., None], axis=-1).sum(-1))) == {0, 1, 2, 3, 4}, "tie orders"
        assert (yp == 0).any() and (yp > 0).any() and (yp < 0).any()
    if N * K > 1:
        assert (nib[-1, -1] == 15).all()
    lines = [('row', i) for s in list(seams[0]) + [0, Hp] for i in (s - 1, s) if 0 <= i < Hp]
    lines += [('col', j) for s in list(seams[1]) + [0, Wp] for j in (s - 1, s) if 0 <= j < Wp]
    for kind, p in lines:
        line = nib[:, :, p, :] if kind == 'row' else nib[:, :, :, p]
        if line.size >= 32 and line.shape[-1] >= 4:       # (a shorter line is all border ties)
            assert {1, 2, 4, 8} <= set(np.unique(line)), (kind, p)
    if Wp >= 8 and Hp >= 8:
        for edge in (nib[:, :, 0], nib[:, :, -1], nib[:, :, :, 0], nib[:, :, :, -1]):
            assert np.isin(edge, (3, 12, 15)).any()


ALL_ROWS = [('wgrad', r) for r in R.WGRAD_ROWS] + [('dgrad', r) for r in R.DGRAD_ROWS]


@pytest.mark.parametrize("fam,row", ALL_ROWS, ids=lambda v: v if isinstance(v, str) else R.row_id(v))
def test_inputs_hold_what_the_rows_need_and_integers_stay_exact(fam, row):
    seams = (R.wgrad_seams if fam == 'wgrad' else R.dgrad_seams)(row.g)
    for integer in (True, False):
        d = R.inputs(row.g, seams, integer)
        inventory(d['mask'], d['yp'], seams)
        if integer:
            for name, top in (('x', 3), ('gp', 3), ('W', 2)):
                assert np.array_equal(d[name], np.round(d[name])) and 0 < np.abs(d[name]).min() and np.abs(d[name]).max() <= top
                assert all((p == 0).all() for p in R.pieces(d[name], 'bf16x3')[1:])
            for act in R.ACTS:
                for yp in (d['yp'], None):
                    m = R.magnitude(d['x'], d['W'], d['mask'], yp, d['gp'], act, R.SLOPE)
                    # terms are multiples of 1 / 4; twice (accumulating a result onto itself) plus the previous value
                    assert all(4 * (2 * v.max() + 7) < 2 ** 24 for v in m.values()), (act, {k: v.max() for k, v in m.items()})
    assert np.float32(R.SLOPE) == R.SLOPE


@pytest.mark.parametrize("g", R.WGRAD_FORWARD + R.DGRAD_FORWARD, ids=str)
def test_forward_masks_hold_ties_and_the_sign_bit(g):
    for integer in (True, False):
        d = R.forward_inputs(g, integer)
        nib = d['mask'] & 15
        assert (nib != 0).all() and (nib == 15).any() and np.isin(nib, (1, 2, 4, 8)).any()
        assert np.array_equal((d['mask'] & 16) != 0, d['yp'] > 0) and d['yp'].dtype == np.float32


# ---- the rows' claims ----
@pytest.mark.parametrize("row", R.WGRAD_ROWS, ids=R.row_id)
def test_weight_gradient_row_reaches_what_it_claims(row):
    N, H, W, K = row.g
    d = desc(row.g, row.view)
    assert d.x_nstride >= H * W and (row.view != 'slice' or d.x_nstride > H * W)
    for act in R.ACTS:
        assert supported(d, act) & 1
    rb = N * (H // 2) * K * (R.T + 1) * 4 // ws_bytes("ghm_conv2d_pool_wgrad_sparse_workspace", d)
    nseg = (W // 2 + 63) // 64
    assert dict(rb=rb, nseg=nseg, items=rb * nseg, S=N * (H // 2) // rb) == row.reaches and rb == R.wgrad_rb(H, W)


def test_weight_gradient_table_covers_the_issue():
    rows = R.WGRAD_ROWS
    by = lambda f: {f(r) for r in rows}
    assert by(lambda r: r.reaches['rb']) == {8, 4, 2, 1}
    assert {(r.reaches['rb'], r.g[1] // 2) for r in rows} >= {(8, 8), (4, 4), (2, 6), (1, 23)}
    at = {(r.g[1], r.g[2]): r.reaches['rb'] for r in rows}
    assert (at[(16, 636)], at[(16, 638)], at[(16, 1024)], at[(2, 2172)]) == (8, 4, 2, 1)
    assert supported(desc(R.WGRAD_UNSERVED)) & 1 == 0 and ws_bytes("ghm_conv2d_pool_wgrad_sparse_workspace", desc(R.WGRAD_UNSERVED)) == 0
    assert by(lambda r: r.g[2] // 2) >= {1, 63, 64, 65}
    assert by(lambda r: r.g[3]) >= {1, 8, 9, 16, 17, 64, 65, 96}
    assert by(lambda r: r.reaches['S']) >= {1, 64, 69}
    items = by(lambda r: r.reaches['items'])
    assert any(i < 4 for i in items) and any(i > 4 and i % 4 for i in items) and any(i > 8 and i % 8 for i in items) and any(i % 8 == 0 for i in items)
    assert by(lambda r: r.view) == {'whole', 'slice', 'offset'}
    with tuning_env(GHM_NO_POOL_SPARSE_BWD='1'):
        assert supported(desc(rows[0].g)) == 0


@pytest.mark.parametrize("row", R.DGRAD_ROWS, ids=R.row_id)
def test_data_gradient_row_reaches_what_it_claims(row):
    N, H, W, K = row.g
    d = desc(row.g, row.view)
    assert supported(d) & 2 and d.x_nstride % 2 == 0
    assert row.reaches == dict(tiles=(-(-(H // 2) // 8), -(-(W // 2) // 32)), rounds=-(-K // 8), kn=(K - 1) % 8 + 1)


def test_data_gradient_table_covers_the_issue():
    by = lambda f: {f(r) for r in R.DGRAD_ROWS}
    assert by(lambda r: r.g[1] // 2) >= {1, 8, 9} and by(lambda r: r.g[2] // 2) >= {1, 32, 33} and by(lambda r: r.g[3]) >= {1, 8, 9, 64}
    assert by(lambda r: r.view) == {'whole', 'slice', 'offset'}
    assert supported(desc(R.DGRAD_REFUSED_K)) & 2 == 0 and supported(desc(R.DGRAD_REFUSED_K)) & 1
    g = R.DGRAD_ROWS[1].g
    assert supported(desc(g, xns=g[1] * g[2] + 1)) & 2 == 0 and supported(desc(g, xns=g[1] * g[2] + 1)) & 1


@pytest.mark.parametrize("row", R.SPLIT_ROWS, ids=R.row_id)
def test_split_row_reaches_what_it_claims(row):
    N, Cc, K, H, W = row.g
    d, lib = split_desc(row.g), load()
    with tuning_env(**row.env):
        assert lib.ghm_conv2d_wgrad_pooled_split_supported(C.byref(d)) == 1
        plan = R.split_plan(row.g, row.env)
        assert dict(plan, hwp=(H // 2) * (W // 2)) == row.reaches
        # the strip count x split count is what the workspace is sized by
        assert ws_bytes("ghm_conv2d_wgrad_split_workspace", d) == N * (W // plan['spx']) * plan['splits'] * Cc * 25 * K * 4
        for pattern in R.FLAG_PATTERNS:
            fl = R.compressed(R.split_inputs(row.g, plan, pattern, True)['mask'], None, np.ones((N, K, H // 2, W // 2), np.float32), 'linear', 0.0, 'bf16x3')[2]
            want = np.zeros((N, H), np.int32)
            want[:, R.flagged_rows(row.g, plan, pattern)] = 1
            assert np.array_equal(fl.reshape(N, H), want), pattern
    with tuning_env(**dict(row.env, GHM_NO_SPARSE_WGRAD='1')):
        assert lib.ghm_conv2d_wgrad_pooled_split_supported(C.byref(d)) == 0


def test_split_table_covers_the_issue():
    assert [r.g for r in R.SPLIT_ROWS] == [(1, 32, 64, 2, 32), (2, 32, 64, 16, 64), (1, 64, 128, 4, 96), (3, 32, 64, 6, 128), (1, 32, 64, 18, 64)]
    assert {r.reaches['spx'] for r in R.SPLIT_ROWS} == {32, 64} and {r.reaches['splits'] for r in R.SPLIT_ROWS} == {1, 2}
    assert R.SPLIT_ROWS[1].env and R.SPLIT_ROWS[0].reaches['hwp'] < 256 < R.SPLIT_ROWS[4].reaches['hwp'] < 512


@pytest.mark.parametrize("row", R.SPLIT_ROWS, ids=R.row_id)
def test_split_integer_inputs_stay_exact(row):
    plan = R.split_plan(row.g, row.env)
    d = R.split_inputs(row.g, plan, 'all', True)
    G = R.dense_grad(d['mask'], d['yp'], d['gp'], 'lrelu', R.SLOPE)
    assert 4 * (2 * R.wgrad64(np.abs(d['x']), np.abs(G)).max() + 7) < 2 ** 24
    assert all((p == 0).all() for p in R.pieces(G.astype(np.float32), 'bf16x3')[1:])


# ---- the calibration of k ----
def measure(fam):
    worst = 0.0
    for row in (R.WGRAD_ROWS if fam == 'wgrad' else R.DGRAD_ROWS):
        seams = (R.wgrad_seams if fam == 'wgrad' else R.dgrad_seams)(row.g)
        d = R.inputs(row.g, seams, False)
        args = (d['mask'], d['yp'], d['gp'], 'lrelu', R.ALPHA)
        ref, M = R.ref(d['x'], d['W'], *args), R.magnitude(d['x'], d['W'], *args)
        if fam == 'wgrad':
            dW, db = R.restate32_wgrad(d['x'], *args)
            w = max(R.worst(dW, ref['dW'], M['dW']), R.worst(db, ref['db'], M['db']))
        else:
            w = R.worst(R.restate32_dgrad(d['W'], *args), ref['dx'], M['dx'])
        print("%s %s: restatement worst %.3f" % (fam, R.row_id(row), w))
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("fam", ['wgrad', 'dgrad'])
def test_frozen_k_is_twice_the_remeasured_restatement(fam):
    w = cached(('k', fam), lambda: measure(fam))
    print("%s: worst %.2f -> k %d" % (fam, w, math.ceil(2 * w)))
    assert R.K_BOUND[fam] == math.ceil(2 * w), (fam, w)
    # n + S + 2 of the smallest row: the weight gradient's n counts pooled elements; a pixel of the data gradient meets the 25
    # arg-max positions within two pixels of it, per filter (all of them where every window is tied)
    n = min(r.g[0] * (r.g[1] // 2) * (r.g[2] // 2) + r.reaches['S'] for r in R.WGRAD_ROWS) if fam == 'wgrad' else min(25 * r.g[3] for r in R.DGRAD_ROWS)
    assert R.K_BOUND[fam] <= n + 2
    assert R.K_BOUND['bf16x3'] == R.S2.K_BOUND[('bf16x3', 'wgrad')] and R.K_BOUND['bf16x2'] == R.S2.K_BOUND[('bf16x2', 'wgrad')]


# ---- what the per-element check sees; whether the older rel-L2 <= 1e-5 lets the same mutation through ----
# name -> (the per-element check fails, the older norm passes), recorded from this test's own printout
MUTATIONS = {
    'row dropped at a band seam': (True, False),
    'tie to the first arg-max only': (True, False),
    'column bit flipped in one window': (True, False),
    'column bit flipped in a window of small gradient': (True, True),
    'slope of the wrong sign on exact-zero yp': (True, False),
    'halo cell dropped at a tile seam': (True, False),
}
MUT_G = (3, 96, 128, 64)            # a geometry of the older test


def _mutants():
    g = MUT_G
    N, H, W, K = g
    d = R.inputs(g, R.wgrad_seams(g), False)
    args = dict(act='lrelu', alpha=R.ALPHA)
    x, Wt, mask, yp, gp = d['x'], d['W'], d['mask'], d['yp'], d['gp']
    ref, M = R.ref(x, Wt, mask, yp, gp, **args), R.magnitude(x, Wt, mask, yp, gp, **args)
    rb = R.wgrad_rb(H, W)
    out = {}
    m1 = mask.copy()
    m1[1, 5, rb, :] &= 16                                                   # the first row of the second band: nothing sent
    out['row dropped at a band seam'] = R.ref(x, Wt, m1, yp, gp, **args)
    low = (mask & 15) & (~(mask & 15) + 1).astype(np.uint8)                 # the lowest set bit
    tied = np.unpackbits((mask & 15)[..., None], axis=-1).sum(-1) > 1
    m2 = mask.copy()
    sel = np.argwhere(tied & (np.arange(K)[None, :, None, None] == 7) & (np.arange(N)[:, None, None, None] == 0))[:1]
    for i in sel:
        m2[tuple(i)] = (mask[tuple(i)] & 16) | low[tuple(i)]                # one tied window of one filter
    out['tie to the first arg-max only'] = R.ref(x, Wt, m2, yp, gp, **args)
    m3 = mask.copy()
    i = tuple(np.argwhere((mask & 15) == 1)[len(mask) // 2])
    m3[i] = (mask[i] & 16) | 2                                              # arg-max moved one column
    out['column bit flipped in one window'] = R.ref(x, Wt, m3, yp, gp, **args)
    # the same mistake in a window whose gradient is 4e-3 of the tensor's rms: below what the norm of 1e-5 can see
    v = np.abs(gp * R.slope_of(mask, yp, **args))
    cand = np.argwhere((mask & 15) == 1)
    j = tuple(cand[np.argmin(np.abs(v[tuple(cand.T)] - 4e-3 * np.sqrt((v * v).mean())))])
    m6 = mask.copy()
    m6[j] = (mask[j] & 16) | 2
    out['column bit flipped in a window of small gradient'] = R.ref(x, Wt, m6, yp, gp, **args)
    zero = np.argwhere((yp == 0) & ((mask & 15) != 0))[:1]
    y4 = yp.copy()
    y4[tuple(zero[0])] = np.float32(1e-30)                                  # 0 taken for positive: slope 1 in place of alpha
    out['slope of the wrong sign on exact-zero yp'] = R.ref(x, Wt, mask, y4, gp, **args)
    # the thread of cell (7, 31) (the last of its tile) never sees its right-hand neighbour, the first cell of the next tile
    m5 = R.ref(x, Wt, mask, yp, gp, **args)
    contrib = mask.copy()
    contrib[:, :, :, :] &= 16
    contrib[0, :, 7, 32] = mask[0, :, 7, 32]
    part = R.ref(x, Wt, contrib, yp, gp, **args)['dx']
    dx5 = ref['dx'].copy()
    dx5[0, 0, 14:16, 62:64] -= part[0, 0, 14:16, 62:64]
    m5['dx'] = dx5
    out['halo cell dropped at a tile seam'] = m5
    return ref, M, out


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_seen_per_element(name):
    ref, M, out = cached('mutants', _mutants)
    got = out[name]
    seen = any(R.worst(got[k], ref[k], M[k]) > R.K_BOUND['dgrad' if k == 'dx' else 'wgrad'] for k in ('dW', 'db', 'dx'))
    norm_passes = all(R.rel(got[k], ref[k]) < R.REL_L2 for k in ('dW', 'db', 'dx'))
    print("%s: worst per element %s, rel-L2 %s -> seen %s, the older norm passes %s"
          % (name, {k: round(R.worst(got[k], ref[k], M[k]), 1) for k in got}, {k: "%.1e" % R.rel(got[k], ref[k]) for k in got}, seen, norm_passes))
    assert seen, name
    assert (seen, norm_passes) == MUTATIONS[name], (name, seen, norm_passes)
