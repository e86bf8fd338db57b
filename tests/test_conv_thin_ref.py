"""CPU checks of tests/conv_thin_ref.py: the reference against torch in float64, the explicit dot products against the
reference, the integer inputs' exactness claims, every row's ``reaches`` claim through the library's host-only queries and the
restated planners (under the row's own tuning environment), the table's coverage, the calibration of k, and -- once per kernel
family -- that the per-element checks see what the whole-tensor norm does not.

Wall time without a GPU: 94 tests in 35 s (the calibration of k 22 s of it, the weight gradient's 7 s; drawing the integer
inputs of the 36 geometries 8 s).
"""
import ctypes as C

import numpy as np
import pytest

from gan_heightmaps_amd import device as D
from gan_heightmaps_amd._lib import call, load, tuning_env
from tests import conv_thin_ref as R

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def desc(g, view='whole'):
    N, Cc, H, W, K, k, s, pad = g
    xs, _, ys = R.shapes(g)
    return D.conv_desc(N, Cc, H, W, K, k, k, s, pad, R.view_layout(xs, view)[1], R.view_layout(ys, view)[1])


def variant(d, kind):
    out = C.create_string_buffer(128)
    call("ghm_conv2d_variant", C.byref(d), kind, out, 128)
    return out.value.decode()


# ---- the reference ----
@pytest.mark.parametrize("g", [(2, 3, 12, 20, 5, 5, 1, 2), (2, 4, 12, 16, 6, 3, 2, 1), (1, 3, 8, 12, 7, 2, 2, 0), (2, 6, 10, 14, 2, 3, 1, 1)], ids=str)
def test_reference_agrees_with_torch_in_float64(g):
    torch = pytest.importorskip("torch")
    N, Cc, H, W, K, k, s, pad = g
    d = R.real_inputs(g)
    x = torch.tensor(d['x'].astype(np.float64), requires_grad=True)
    Wt = torch.tensor(d['W'].astype(np.float64), requires_grad=True)
    y = torch.nn.functional.conv2d(x, torch.flip(Wt, (2, 3)), torch.tensor(d['b'].astype(np.float64)), stride=s, padding=pad)
    y.backward(torch.tensor(d['dy'].astype(np.float64)))
    for kind, want in (('fwd', y.detach().numpy()), ('dgrad', x.grad.numpy()), ('wgrad', Wt.grad.numpy())):
        got = R.ref(kind, g, d['x'], d['W'], d['b'] if kind == 'fwd' else None, d['dy'])
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), kind
    # the explicit dot products that restate32 sums are this reference, element by element (borders and corners), and
    # sum |a| |b| is M; the weight gradient's planes likewise, on both thin sides
    for kind in ('fwd', 'dgrad'):
        idx = R.sample_idx(kind, g, count=300)
        A = d['x'] if kind == 'fwd' else d['dy']
        a, b = R.terms(kind, g, A.astype(np.float64), d['W'].astype(np.float64), idx)
        ref, m = R.ref(kind, g, d['x'], d['W'], None, d['dy']), R.M(kind, g, d['x'], d['W'], None, d['dy'])
        assert np.abs((a * b).sum(1) - R.at(ref, idx)).max() <= 1e-12 * m.max()
        assert np.abs(np.abs(a * b).sum(1) - R.at(m, idx)).max() <= 1e-12 * m.max()
    assert R.wgrad_side(g) == (1 if Cc <= 4 else 2) and (Cc <= 4 or s == 1)
    ref, m = R.ref('wgrad', g, d['x'], None, None, d['dy']), R.M('wgrad', g, d['x'], None, None, d['dy'])
    for tap in R.wgrad_taps(g):
        assert np.abs(R.wgrad_at(g, d['x'], d['dy'], tap) - ref[R.wgrad_index(g, tap)]).max() <= 1e-12 * m.max(), tap
        assert np.abs(R.wgrad_at(g, d['x'], d['dy'], tap, absolute=True) - m[R.wgrad_index(g, tap)]).max() <= 1e-12 * m.max(), tap


def test_pool_reference_mask_layout():
    y = np.array([[[[1., 3., -1., -1.], [3., 2., -1., -2.]]]])
    p, m = R.pool_ref(y)
    assert p.tolist() == [[[[3., -1.]]]]
    assert m.tolist() == [[[[2 | 4 | 16, 1 | 2 | 4]]]]          # ties at (0, 1) and (1, 0): bits 1 and 2, positive; three-way tie, negative


# ---- the integer inputs ----
@pytest.mark.parametrize("g", sorted({r.g for r in R.ROWS}), ids=str)
def test_integer_inputs_keep_every_partial_sum_exact(g):
    d = R.int_inputs(g)
    for name, top in (('x', 3), ('dy', 3), ('W', 2), ('b', 4), ('bc', 4)):
        a = d[name]
        assert np.array_equal(a, np.round(a)) and (a != 0).all() and np.abs(a).max() <= top, name
    for kind in ('fwd', 'dgrad', 'wgrad'):
        assert np.abs(d['prev'][kind]).max() <= 7
        assert 2 * R.int_magnitude(kind, g) < 2 ** 24, kind          # x 2: the accumulate form on top of itself
        assert 4 * R.int_magnitude(kind, g) < 2 ** 26                # times the slope 0.25: quarter-integers, exact
    assert np.float32(R.SLOPE) == R.SLOPE


# ---- the rows' claims ----
def reached(row):
    """what the library's host-only queries (planning with 256 CUs) and the restated planners say this row runs"""
    d, lib, g = desc(row.g, row.view), load(), row.g
    if row.kernel == 'pool':
        assert lib.ghm_conv2d_pool_supported(C.byref(d), D.ACT_CODES['lrelu'], D.DTYPE_CODES['f32']) == 1 and g[1] <= 4
        return dict(variant='pool', plan=R.pool_reaches(g, row.env))
    v = variant(d, R.KIND_CODE[row.kind])
    if row.kernel == 'fanout':
        return dict(variant=v, plan=R.fanout_reaches(row.kind, g, row.env))
    if row.kernel == 'fanin_s1':
        return dict(variant=v, form=(g[5], g[1] if row.kind == 'fwd' else g[4]))
    if row.kernel == 'fanin_s2':
        return dict(variant=v, form=(g[5], g[1]))
    assert row.kernel == 'thin_wgrad'
    return dict(variant=v, plan=R.wgrad_reaches(g), side=R.wgrad_side(g))


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_row_reaches_what_it_claims(row):
    assert row.view in R.VIEWS
    with tuning_env(**row.env):
        got = reached(row)
    assert got == row.reaches, (got, row.reaches)
    if R.multi_key(row) in R.MULTI:
        assert R.iterations(row) > R.MULTI[R.multi_key(row)] * R.CUS, row
    elif row.kernel in ('fanout', 'pool', 'thin_wgrad'):
        assert R.iterations(row) <= R.CUS           # every other row: one iteration per block (the control of the MULTI rows)


@pytest.mark.parametrize("q", R.Q_ROWS, ids=str)
def test_q_rows_are_served_by_the_fp32_fan_out(q):
    kind, g, ks = q
    d, lib = desc(g), load()
    with tuning_env(**R.Q_ENV):
        for mode in R.Q_MODES:
            assert lib.ghm_thin_fwd_q_supported(C.byref(d), D.ACT_CODES['lrelu'], int(kind == 'pool'), D.DTYPE_CODES[mode]), mode
            if kind == 'pool' and mode in ('bf16', 'f16'):
                assert not lib.ghm_thin_pool_lp_served(C.byref(d), D.ACT_CODES['lrelu'], R.SLOPE, D.DTYPE_CODES[mode])
    assert (R.fanout_reaches('fwd', g)[0] if kind == 'fwd' else R.pool_reaches(g)[0]) == ks
    assert kind == 'fwd' or (R.pool_reaches(g)[1] == 2 and ks <= 13)


def test_misaligned_rows_would_be_taken_by_the_thin_kernels_if_aligned():
    """the guard's rows: aligned, the same descriptor goes to the fan-out kernel (so the 4-byte offset is what turns it away)"""
    for kind, g in R.MISALIGNED:
        d = desc(g)
        if kind == 'pool':
            assert load().ghm_conv2d_pool_supported(C.byref(d), D.ACT_CODES['lrelu'], D.DTYPE_CODES['f32']) == 1
        else:
            assert variant(d, R.KIND_CODE[kind]) == 'fanout_kernel<%s>' % kind


def _cover(row):
    r = row.reaches
    if row.kernel == 'fanout':
        return {('fanout', r['plan'][0], 'plain'), ('fanout', r['plan'][0], 'ACC')}
    if row.kernel == 'pool':
        return {('pool', 'WS%d' % r['plan'][1])}
    if row.kernel in ('fanin_s1', 'fanin_s2'):
        return {(row.kernel,) + r['form']}
    return {('thin_wgrad',) + r['plan'][:2], ('thin_wgrad', 'side', r['side'])}


def test_table_covers_every_instantiation():
    have = set().union(*[_cover(r) for r in R.ROWS])
    have |= {('fanout', ks, 'QOUT') for kind, g, ks in R.Q_ROWS if kind == 'fwd'} | {('pool', 'QOUT') for kind, g, ks in R.Q_ROWS if kind == 'pool'}
    assert R.COVERAGE <= have, sorted(R.COVERAGE - have, key=str)
    for kernel in ('fanout', 'fanin_s1', 'fanin_s2', 'thin_wgrad', 'pool'):
        rows = [r for r in R.ROWS if r.kernel == kernel]
        assert {r.view for r in rows} == set(R.VIEWS), kernel
        assert any(r.view == 'slice' and r.g[0] >= 2 for r in rows), kernel            # a sample-stride mistake shows
    for kind in ('fwd', 'dgrad', 'dgrad_t'):
        assert {r.view for r in R.ROWS if r.kernel == 'fanout' and r.kind == kind} == set(R.VIEWS), kind
    assert set(R.MULTI) <= {R.multi_key(r) for r in R.ROWS}
    assert {k for k, _ in R.MISALIGNED} == {'fwd', 'dgrad', 'dgrad_t', 'pool'}


# ---- k ----
def measure_one(kind, g):
    d = R.real_inputs(g)
    if kind == 'wgrad':
        w = 0.0
        for tap in R.wgrad_taps(g):
            w = max(w, R.worst(R.wgrad_at(g, d['x'], d['dy'], tap, np.float32), R.wgrad_at(g, d['x'], d['dy'], tap),
                               R.wgrad_at(g, d['x'], d['dy'], tap, absolute=True)))
        return w
    b, idx = R.bias_of(kind, d), R.sample_idx(kind, g)
    A = d['x'] if kind == 'fwd' else d['dy']
    ta, tb = R.terms(kind, g, A.astype(np.float64), d['W'].astype(np.float64), idx)
    bias = b.astype(np.float64)[idx[:, 1]]
    return R.worst(R.restate32(kind, g, d['x'], d['W'], b, d['dy'], idx), (ta * tb).sum(1) + bias, np.abs(ta * tb).sum(1) + np.abs(bias))


def measure(key):
    gs = sorted({(R.base_kind(r.kind), r.g) for r in R.ROWS if R.family_key(r) == key})
    return max(cached(('k', kind, g), lambda: measure_one(kind, g)) for kind, g in gs)


@pytest.mark.parametrize("key", sorted(R.K_BOUND), ids=lambda k: "%s-%s" % k)
def test_k_is_twice_the_sequential_fp32_restatement(key):
    w = measure(key)
    k = R.K_BOUND[key]
    print("%s %s: restate32 worst %.2f x 2^-24 M -> k = %d (frozen %d)" % (key + (w, int(np.ceil(2 * w)), k)))
    assert k == int(np.ceil(2 * w)), (key, w, k)
    for r in R.ROWS:
        if R.family_key(r) == key:
            S = 8 + R.CUS if r.kernel == 'thin_wgrad' else (r.g[5] ** 2 if r.kernel == 'fanin_s1' else 1)
            assert k <= R.n_products(r.kind, r.g) + S + 2, r


# ---- sensitivity ----
def weakest(E, ref):
    """the largest power of two f for which the mistake f E is inside the whole-tensor norm bound"""
    f = 1.0
    while np.linalg.norm(f * E) / np.linalg.norm(ref) >= R.REL_L2:
        f /= 2
    return f


def test_per_element_checks_see_what_the_norm_does_not():
    """Three mistakes, each at full strength (f = 1: what a wrong mask or a wrong hand-over does) and at the largest power of two
    f at which rel-L2 stays under 1e-5 (how faint it must be for the older tests to pass it).  The per-element check fails
    both.  With finite neighbours; in the GPU module what lies outside a view is NaN and the first fails outright.
    (a) fan-out forward: one border tap's products missing in the first output row of one image;
    (b) fanin_s2: the dy row under the bottom border taken from the next sample instead of zero;
    (c) thin_wgrad on a geometry with several rows per block: one big-tensor row's contribution missing from one tap."""
    # (a)
    g = (2, 1, 128, 128, 64, 5, 1, 2)
    d = R.real_inputs(g)
    ref, m = R.ref('fwd', g, d['x'], d['W'], d['b'], None), R.M('fwd', g, d['x'], d['W'], d['b'], None)
    k = R.K_BOUND[('fanout', 'fwd')]
    assert R.worst(ref.astype(np.float32), ref, m) <= 1
    E = np.zeros_like(ref)          # output row 0 reads input row 0 through tap row a = pad (flipped filter index k - 1 - pad)
    E[1, :, 0, :] = -d['W'].astype(np.float64)[:, 0, 2, 2][:, None] * d['x'].astype(np.float64)[1, 0, 0][None, :]
    for f in (1.0, weakest(E, ref)):
        bad = (ref + f * E).astype(np.float32)
        w, r = R.worst(bad, ref, m), R.rel(bad, ref)
        print("(a) f = %.3g: %.1f x 2^-24 M (k = %d), rel-L2 %.2e" % (f, w, k, r))
        assert w > k and (f == 1.0 or r < R.REL_L2)
    # (b)
    g = (2, 3, 192, 192, 256, 3, 2, 1)
    d = R.real_inputs(g)
    ref, m = R.ref('dgrad', g, None, d['W'], d['bc'], d['dy']), R.M('dgrad', g, None, d['W'], d['bc'], d['dy'])
    k = R.K_BOUND[('fanin_s2', 'dgrad')]
    ghost = np.zeros_like(d['dy'], dtype=np.float64)            # what the last output row of sample 0 gains from sample 1's first dy row:
    gpad = (g[0], g[1], g[2] + 2, g[3], g[4], g[5], g[6], g[7])  # the same transposed filter on a map one dy row taller
    tall = np.concatenate([ghost[:1], d['dy'][1:, :, :1].astype(np.float64)], axis=2)
    E = np.zeros_like(ref)
    E[0] = R.ref('dgrad', gpad, None, d['W'], None, tall)[0, :, :g[2]]
    assert (E[0, :, :-1] == 0).all() and (E[0, :, -1] != 0).all()        # only the last row (2 Ho - 1 meets dy row Ho through one tap row)
    for f in (1.0, weakest(E, ref)):
        bad = (ref + f * E).astype(np.float32)
        w, r = R.worst(bad, ref, m), R.rel(bad, ref)
        print("(b) f = %.3g: %.1f x 2^-24 M (k = %d), rel-L2 %.2e" % (f, w, k, r))
        assert w > k and (f == 1.0 or r < R.REL_L2)
    # (c)
    g = (3, 1, 96, 256, 64, 5, 1, 2)
    d = R.real_inputs(g)
    ref, m = R.ref('wgrad', g, d['x'], None, None, d['dy']), R.M('wgrad', g, d['x'], None, None, d['dy'])
    k = R.K_BOUND[('thin_wgrad', 'wgrad')]
    tap = (0, 1, 3)
    big, plane = R.wgrad_planes(g, d['x'], d['dy'], tap)
    n, row = int(np.argmax(np.abs(d['x']).mean(axis=(1, 2, 3)))), 40          # row 40 + 256 of the brightest sample: a block's second row
    E = np.zeros_like(ref)
    E[R.wgrad_index(g, tap)] = -(big[n, :, row].astype(np.float64) * plane[n, row].astype(np.float64)[None, :]).sum(1)
    for f in (1.0, weakest(E, ref)):
        bad = (ref + f * E).astype(np.float32)
        w, r = R.worst(bad, ref, m), R.rel(bad, ref)
        print("(c) f = %.3g: %.1f x 2^-24 M (k = %d), rel-L2 %.2e" % (f, w, k, r))
        assert w > k and (f == 1.0 or r < R.REL_L2)
