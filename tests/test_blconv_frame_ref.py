"""CPU checks of tests/blconv_frame_ref.py: the frame-only float64 definitions against the literal up-sample and convolve and
against each other as adjoints, the explicit line products against them, every row's split claim at 256 CUs (mirror and the
library's own host-only query), the coverage of the table, the integer inputs' magnitude bound and the calibration of k."""
import numpy as np
import pytest

from oracle import ops as O
from tests import blconv_frame_ref as R

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


SMALL = [(2, 3, 4, 5, 7), (1, 2, 3, 2, 2), (1, 2, 2, 2, 3), (2, 4, 5, 3, 2), (1, 3, 2, 16, 15)]


def _draw(g):
    xs, ws, ys = R.shapes(g)
    r = np.random.RandomState(sum(g))
    return r.randn(*xs), r.randn(*ws), r.randn(*ys), r.randn(ws[0])


# ---- the definitions ----
@pytest.mark.parametrize("g", SMALL, ids=str)
def test_frame_plus_main_plus_bias_is_the_literal_layer(g):
    x, W, dy, b = _draw(g)
    N, C, K, n1, n2 = g
    lit = O.conv2d_fwd(O.bilinear_up2_fwd(x), W, b, 1, 1)
    got = R.frame_fwd(x, W) + O.bilinear_conv_main(x, W).reshape(N, 4 * K, n1, n2) + np.tile(b, 4).reshape(1, 4 * K, 1, 1)
    assert np.abs(R.to_hi(got) - lit).max() <= 1e-12 * np.abs(lit).max()
    assert np.array_equal(R.to_pp(R.to_hi(got)), got)
    assert not R.frame_fwd(x, W)[~R.border_pp(g)].any()                       # exactly zero off the border
    assert np.abs(R.frame(x) - O.bilinear_conv_frame(x)).max() <= 1e-14 * np.abs(x).max()
    assert (R.M('fwd', x, W, dy) >= np.abs(R.frame_fwd(x, W)) * (1 - 1e-12)).all()


@pytest.mark.parametrize("g", SMALL, ids=str)
def test_the_two_gradients_are_the_adjoints(g):
    x, W, dy, _ = _draw(g)
    lhs = (R.frame_fwd(x, W) * dy).sum()
    scale = (R.M('fwd', x, W, dy) * np.abs(dy)).sum()
    assert abs(lhs - (x * R.frame_dgrad(dy, W)).sum()) <= 1e-12 * scale
    assert abs(lhs - (W * R.frame_wgrad(x, dy)).sum()) <= 1e-12 * scale
    assert not R.frame_dgrad(dy, W)[~R.border_coarse(g)].any()
    # the interior of dy does not matter
    assert np.array_equal(R.frame_dgrad(np.where(R.border_pp(g), dy, 0), W), R.frame_dgrad(dy, W))
    assert np.array_equal(R.frame_wgrad(x, np.where(R.border_pp(g), dy, 0)), R.frame_wgrad(x, dy))
    # M is the same computation on absolute values: it dominates, and is its own adjoint pairing
    for kind in R.KINDS:
        assert (R.M(kind, x, W, dy) >= np.abs(R.ref(kind, x, W, dy)) * (1 - 1e-12)).all(), kind
    assert abs((R.M('fwd', x, W, dy) * np.abs(dy)).sum() - (np.abs(x) * R.M('dgrad', x, W, dy)).sum()) <= 1e-12 * scale
    assert abs((R.M('fwd', x, W, dy) * np.abs(dy)).sum() - (np.abs(W) * R.M('wgrad', x, W, dy)).sum()) <= 1e-12 * scale


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("g", [(2, 3, 4, 5, 7), (1, 2, 3, 2, 2), (2, 4, 5, 3, 2), (1, 3, 2, 16, 15)], ids=str)
def test_line_products_are_the_reference_at_every_border_pixel(g, kind):
    """the six jobs on the four lines, as the kernels form them (tests/blconv_frame_ref.terms), sum to the float64 frame-only
    result at every border pixel, and sum |a| |b| is M"""
    x, W, dy, _ = _draw(g)
    idx = R.sample_idx(kind, g, count=200)
    a, b = R.terms(kind, g, x, W, dy, idx)
    assert a.dtype == np.float64 and b.dtype == np.float64
    m = R.at(kind, R.M(kind, x, W, dy), idx)
    assert np.abs((a * b).sum(1) - R.at(kind, R.ref(kind, x, W, dy), idx)).max() <= 1e-12 * m.max()
    # a line value 0.5 (x[m] + x[m + 1]) may cancel, M (from |x|) does not: sum |a| |b| <= M, with equality once x >= 0
    assert (np.abs(a * b).sum(1) <= m * (1 + 1e-12)).all()
    a, b = R.terms(kind, g, np.abs(x), W, dy, idx)
    assert np.abs(np.abs(a * b).sum(1) - m).max() <= 1e-12 * m.max()
    assert a.shape[1] >= R.n_products(kind, g)                  # (the kernels multiply the structural zeros too)


def test_buffer_restatements_hold_the_frame():
    """FL is the frame itself where one line lies, DYL the border of dy; both in float32 without any rounding but 0.5 (a + b)"""
    g = (2, 3, 4, 5, 7)
    x, W, dy, _ = _draw(g)
    FL, F = R.lines(x, np.float64), O.bilinear_conv_frame(x)
    n1, n2 = g[3:]
    assert FL.shape == (2, 4, 3, 32) and not FL[..., 2 * max(n1, n2) + 2:].any()
    assert np.allclose(FL[:, 0, :, 1:2 * n2], F[:, :, 0, 1:2 * n2], atol=1e-15)   # fine row -1 between the crossing lines 2 and 3
    assert np.allclose(FL[:, 2, :, :2 * n1 + 2], F[:, :, :, 0], atol=1e-15)       # fine column -1: lines 0 and 1 have a zero ring
    assert np.allclose(FL[:, 1, :, 2 * n2] + FL[:, 3, :, 2 * n1], F[:, :, 2 * n1, 2 * n2], atol=1e-15)     # two lines meet
    x32 = x.astype(np.float32)
    assert np.abs(R.lines(x32) - R.lines(x32, np.float64)).max() <= 2.0 ** -24 * np.abs(x32).max()
    DYL = R.dyl(dy.astype(np.float32))
    assert DYL.shape == (6, 2, 4, 64) and np.count_nonzero(DYL) == 2 * 4 * 3 * (2 * n1 + 2 * n2)
    s = R.frame_sizes(g)
    assert (s['fl_floats'], s['dyl_floats']) == (2 * (2 * 4 * 3 * 32 + 64), 2 * 6 * 2 * 4 * 64)


# ---- the rows ----
@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row_reaches_what_it_claims(row):
    from gan_heightmaps_amd._lib import load
    import ctypes as C
    assert R.plan(row.g)['splits'] == row.splits
    out = (C.c_int32 * 3)()
    assert load().ghm_blconv_frame_splits(None, *row.g, out) == 0           # host only; plans with 256 CUs without a device
    assert tuple(out) == row.splits
    s = R.frame_sizes(row.g)
    a, b = C.c_int64(), C.c_int64()
    assert load().ghm_blconv_frame_sizes(*row.g, C.byref(a), C.byref(b)) == 0
    assert (s['fl_floats'], s['dyl_floats']) == (a.value, b.value)
    assert all(v in R.VIEWS for v in row.views) and sum(v != 'whole' for v in (row.views[0], row.views[1], row.views[3])) >= 1
    assert max(np.prod(sh) for sh in R.shapes(row.g)) <= 2 ** 23


def test_table_reaches_every_split_path():
    have = set().union(*(R.cover(r.g) for r in R.ROWS))
    assert R.COVERAGE <= have, sorted(R.COVERAGE - have, key=str)
    plans = {r.g: R.plan(r.g) for r in R.ROWS}
    assert [hi - lo for lo, hi in plans[(1, 256, 128, 2, 3)]['ranges'][0]] == [86, 86, 84]
    assert [hi - lo for lo, hi in plans[(1, 256, 128, 2, 3)]['ranges'][1]] == [44, 44, 40]
    assert [hi - lo for lo, hi in plans[(1, 1024, 512, 2, 2)]['ranges'][0]] == [94] * 10 + [84]
    assert [hi - lo for lo, hi in plans[(1, 192, 32, 2, 2)]['ranges'][0]] == [96, 96]
    # the tile-edge geometries: LP == 2 n + 4, the data gradient's and the forward's position tile exactly full
    assert plans[(1, 32, 32, 14, 14)]['LP'] == 2 * 14 + 4 == 32
    assert plans[(1, 32, 32, 15, 15)]['used'] == (1, 1) and 2 * 15 + 2 == 32
    assert plans[(1, 32, 32, 16, 15)]['used'] == (1, 2) and 2 * 16 == 32
    assert plans[(4, 32, 32, 48, 48)]['used'] == (3, 4) and plans[(2, 32, 32, 31, 130)]['used'] == (9, 9)
    assert plans[(4, 32, 32, 12, 84)]['LP'] == 192 and plans[(2, 32, 32, 31, 130)]['LP'] == 288
    # (4, 32, 32, 12, 84): the npmin / 4 cap is met exactly, every wave of every split owns ONE pair of the short part
    assert R.bl_splits(2 * 4 * (12 + 84), 9, R.CUS) == 3 == 12 // 4
    for v in range(3):                                                      # every layout for every tensor
        assert {r.views[v] for r in R.ROWS} == set(R.VIEWS)
    assert any(min(r.g[3:]) >= 3 for r in R.ROWS) and any(min(r.g[3:]) == 2 for r in R.ROWS)      # dx with and without interior


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_integer_inputs_stay_exact(row):
    g = row.g
    d = R.int_inputs(g)
    assert np.array_equal(d['x'] % 4, np.zeros_like(d['x'])) and np.abs(d['x']).max() <= 16
    for a in (d['x'], d['W'], d['dy']) + tuple(d['prev'].values()):
        assert np.array_equal(a, np.round(a)) and (a == 0).any() and (a > 0).any() and (a < 0).any()
    FL = R.lines(d['x'])
    assert np.array_equal(FL, np.round(FL)) and np.abs(FL).max() <= 8
    for kind in R.KINDS:
        m = R.M(kind, d['x'], d['W'], d['dy'], prev=d['prev'][kind])
        assert m.max() <= R.int_magnitude(kind, g), kind
        assert 4 * R.int_magnitude(kind, g) < 2 ** 24, kind             # the fold's quarters of integers are exact too
        ref = R.ref(kind, d['x'], d['W'], d['dy'])
        assert np.array_equal(4 * ref, np.round(4 * ref)), kind


# ---- k ----
def measure(kind):
    worst_k = 0.0
    for row in R.ROWS:
        g = row.g

        def one():
            d = R.real_inputs(g)
            idx = R.sample_idx(kind, g)
            prev = d['prev'][kind]
            ref = R.at(kind, R.ref(kind, d['x'], d['W'], d['dy']) + prev, idx)
            m = R.at(kind, R.M(kind, d['x'], d['W'], d['dy'], prev), idx)
            return R.worst(R.restate32(kind, g, d['x'], d['W'], d['dy'], prev, idx), ref, m)
        worst_k = max(worst_k, cached(('k', kind, g), one))
    return worst_k


@pytest.mark.parametrize("kind", R.KINDS)
def test_k_is_twice_the_sequential_fp32_restatement(kind):
    w = measure(kind)
    k = R.K_BOUND[kind]
    print("%s: restate32 worst %.2f x 2^-24 M -> k = %d (frozen %d)" % (kind, w, int(np.ceil(2 * w)), k))
    assert k == int(np.ceil(2 * w)), (kind, w, k)
    for row in R.ROWS:
        s = row.splits[R.KINDS.index(kind)]
        assert 1 <= R.bound(kind, row.g, s) <= R.n_products(kind, row.g) + s + 4, row
