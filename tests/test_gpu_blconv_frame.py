"""The frame entry points of csrc/conv_bilinear.hip (ghm_blconv_frame_fwd / _gather / _dgrad / _wgrad: the border term of every
BilinearUpsample2DLayer(2) -> 3x3 convolution stage, always fp32) in isolation, per element and inside canary views, against
the frame-only float64 reference of tests/blconv_frame_ref.py, at its rows: every split count of the forward and data-gradient
GEMMs (1, 2, 3 ragged, 4, 8, 11), of the weight gradient (direct add, 2, 3) and the position-tile edges n = 14, 15, 16
(tests/test_blconv_frame_ref.py checks the rows' claims, the reference, the inputs and the bound on the CPU).

Per row:
  plan      Ops.blconv_frame_splits (the functions the launches take their counts from) equals the mirror at the device's CU
            count; after the last row the module fails unless every split path of R.COVERAGE has been reached -- a device
            without 256 CUs shows up as a lost path, not as a weaker run;
  layout    FL and DYL are buffers of exactly ghm_blconv_frame_sizes floats between canaries; x, the parity-planar y, dy and
            dx are views (whole / channel slice / offset start) inside NaN-canary allocations; the pixels the frame does not
            own -- the interior of y and dy (everything but fine rows {0, H-2, H-1} and columns {0, W-2, W-1}) and the interior
            of dx -- hold the canary pattern itself: reading one poisons a result, writing one is seen;
  buffers   after the forward call FL and FLt equal the fp32 restatement bit for bit and the 64-float pads keep the canary;
            after the gather DYL and DYLt do, with all their zeros;
  integers  small-integer inputs (every partial sum exact): forward, data gradient and weight gradient onto a border of known
            integers equal previous + float64 reference BIT FOR BIT; GHM_BLCONV_NO_WT=1 gives the same bits;
  reals     |got - ref| <= k 2^-24 M per element (k, M: tests/blconv_frame_ref.py); a repeated call gives identical bits; the
            result is exactly fl32(previous + increment), the increment being what the same call adds onto zeros;
  nothing else moves: no canary changes, x, dy, the weights, FL and DYL are bit-unchanged by the calls that read them, every
            written value is finite.

Measured on the MI355X (the module prints this table when it finishes): max over all rows of |got - ref| / (2^-24 M) against
the asserted k, and the number of comparisons (bit-exact ones included):
  forward          4.696 of 10   (60)
  data gradient    1.894 of 14   (75)
  weight gradient  5.700 of  9   (60)
Every integer comparison was bit-exact at every split count, with and without the transposed weight copy; FL, FLt, DYL and DYLt
equalled their restatements bit for bit on every row, n = 14 (over-read into the pad), 15 and 16 included; every result was
exactly fl32(previous + increment), every repeated call bit-identical; no canary, pad or interior pixel changed, no result
depended on a pixel outside the border: no kernel needed a fix.  With the sum over the splits dropped from
bl_scatter_fwd_kernel (a scratch build, run once) test_integers and test_reals failed on exactly the five rows whose forward
splits -- (1, 192, 32, 2, 2), (1, 256, 128, 2, 3), (2, 352, 96, 3, 2), (1, 1024, 512, 2, 2), (4, 1024, 512, 4, 4) -- and
test_bilinear_conv3_collapsed_onto_the_coarse_grid (tests/test_gpu_ops.py) still passed its six earlier cases and failed the
two added ones.
Wall time on the MI355X: 46 tests in 3.6 s (2.9 s between the fixture's start and end), next to tests/test_gpu_conv_s2.py's 1.8 s.
"""
import functools

import numpy as np
import pytest

from gan_heightmaps_amd._lib import tuning_env
from tests import blconv_frame_ref as R
from tests import canary
from tests import elementwise_q_ref as Q

pytestmark = pytest.mark.gpu

REACHED = set()
_REF = {}
CANARY32 = np.uint32(Q.CANARY * 0x10001)
# (no second figure is asserted: the bound of a split product is per element; a bit-exact comparison of written values holds
# their finiteness too)
LEDGER = canary.Ledger(lambda kind, w, r, n: "measured %-6s worst k %6.3f of %2d  (%d comparisons)" % (kind, w, R.K_BOUND[kind], n),
                       rel_limit=None, order=lambda m: [kind for kind in R.KINDS if kind in m])
gpu, mem = canary.fixtures(LEDGER, _REF)
cached = functools.partial(canary.cached, _REF)
V, Raw = canary.View.named, canary.Bytes.rounded
clean, unchanged, note, exact = canary.clean, canary.unchanged, LEDGER.note, LEDGER.exact


class PV(canary.View):
    """a V of which only the pixels ``owned`` belong to the tensor: the others hold the canary pattern and count as outside"""

    def __init__(self, gpu, shape, view, data, owned):
        super().__init__(gpu, shape, R.view_layout(shape, view))
        self.owned = np.ascontiguousarray(np.broadcast_to(owned, shape))
        bits = np.ascontiguousarray(data, np.float32).reshape(shape).view(np.uint32).copy()
        bits[~self.owned] = CANARY32
        self.set(bits.view(np.float32))
        el0, ns, total = R.view_layout(shape, view)
        m = np.zeros((total, 2), bool)
        for n in range(shape[0]):
            m[el0 + n * ns:el0 + n * ns + self.owned[n].size] = self.owned[n].reshape(-1, 1)
        self.inside = m.reshape(-1)

    def values(self):
        """the owned pixels; the others must still hold the canary"""
        got = self.numpy()
        assert (got.view(np.uint32)[~self.owned] == CANARY32).all(), "a pixel the frame does not own was written"
        return got[self.owned]


class Frame:
    """the operands of one row on the device, and the four calls"""

    def __init__(self, gpu, row, d):
        self.gpu, self.row, self.g, self.d = gpu, row, row.g, d
        dev, ops, D = gpu
        N, C, K, n1, n2 = row.g
        xs, ws, ys = R.shapes(row.g)
        self.sizes = R.frame_sizes(row.g)
        assert ops.blconv_frame_sizes(*row.g) == (self.sizes['fl_floats'], self.sizes['dyl_floats'])
        self.x = V(gpu, xs, row.views[0], d['x'])
        self.wp = Raw(gpu, 4 * 9 * C * K, D.pack_conv_w(d['W']).ravel())
        self.dy = PV(gpu, ys, row.views[2], d['dy'], R.border_pp(row.g))
        self.FL, self.DYL = Raw(gpu, 4 * self.sizes['fl_floats']), Raw(gpu, 4 * self.sizes['dyl_floats'])
        assert self.FL.nbytes == 4 * self.sizes['fl_floats'] and self.DYL.nbytes == 4 * self.sizes['dyl_floats']
        self.inputs, self.outs = [self.x, self.wp, self.dy], []

    def fwd(self, prev):
        y = PV(self.gpu, R.shapes(self.g)[2], self.row.views[1], prev, R.border_pp(self.g))
        self.gpu[1].blconv_frame_fwd(self.x.t, self.wp.t, y.t, self.g[2], self.FL.t)
        self.outs.append(y)
        return y.values()

    def check_lines(self):
        """FL | 64 floats | FLt | 64 floats, then FL joins the inputs"""
        s, buf = self.sizes, self.FL.numpy().view(np.uint32)
        fl = R.lines(self.d['x'])
        assert np.array_equal(buf[:s['fl']], fl.ravel().view(np.uint32)), "FL differs from its fp32 restatement"
        assert np.array_equal(buf[s['flt_at']:s['flt_at'] + s['fl']], R.transposed(fl).ravel().view(np.uint32)), "FLt differs"
        assert (buf[s['fl']:s['flt_at']] == CANARY32).all() and (buf[s['flt_at'] + s['fl']:] == CANARY32).all(), "a pad was written"
        self.FL.snapshot()
        self.inputs.append(self.FL)

    def gather(self):
        s = self.sizes
        self.gpu[1].blconv_frame_gather(self.dy.t, self.g[1], self.g[2], self.DYL.t)
        buf = self.DYL.numpy().view(np.uint32)
        dyl = R.dyl(np.where(R.border_pp(self.g), self.d['dy'], np.float32(0)))
        assert np.array_equal(buf[:s['dyl']], dyl.ravel().view(np.uint32)), "DYL differs from its fp32 restatement"
        assert np.array_equal(buf[s['dylt_at']:], R.transposed(dyl).ravel().view(np.uint32)), "DYLt differs"
        self.DYL.snapshot()
        self.inputs.append(self.DYL)

    def dgrad(self, prev):
        dx = PV(self.gpu, R.shapes(self.g)[0], self.row.views[3], prev, R.border_coarse(self.g))
        self.gpu[1].blconv_frame_dgrad(self.DYL.t, self.wp.t, dx.t, self.g[2])
        self.outs.append(dx)
        return dx.values()

    def wgrad(self, prev):
        N, C, K, n1, n2 = self.g
        D = self.gpu[2]
        dwp = Raw(self.gpu, 4 * 9 * C * K, D.pack_conv_w(prev).ravel())
        self.gpu[1].blconv_frame_wgrad(self.DYL.t, self.FL.t, dwp.t, N, C, K, n1, n2)
        self.outs.append(dwp)
        return D.unpack_conv_w(dwp.numpy(), K, C, 3, 3).ravel()

    def settle(self, what):
        unchanged(what, *self.inputs)
        clean(what, *self.outs)


def references(row, d, key):
    """{kind: (float64 frame-only result, M without the previous value)} at the owned elements, cached per row"""
    def make():
        dyb = np.where(R.border_pp(row.g), d['dy'], np.float32(0))          # (the interior of dy is canary on the device)
        own = {'fwd': R.border_pp(row.g), 'dgrad': R.border_coarse(row.g), 'wgrad': np.ones(R.shapes(row.g)[1], bool)}
        return {k: (R.ref(k, d['x'], d['W'], dyb)[own[k]], R.M(k, d['x'], d['W'], dyb)[own[k]], d['prev'][k][own[k]]) for k in R.KINDS}
    return cached((key, row.g), make)


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_plan(gpu, row):
    dev, ops, D = gpu
    cus = dev.info()['num_cu']
    got = ops.blconv_frame_splits(*row.g)
    assert got == R.plan(row.g, cus)['splits'], (got, cus)
    if cus == R.CUS:
        assert got == row.splits
    REACHED.update(R.cover(row.g, cus))


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_integers(gpu, mem, row):
    d = cached(('int', row.g), lambda: R.int_inputs(row.g))
    refs = references(row, d, 'iref')
    f = Frame(gpu, row, d)
    want = {k: (p.astype(np.float64) + r).astype(np.float32) for k, (r, m, p) in refs.items()}
    exact('fwd', f.fwd(d['prev']['fwd']), want['fwd'], "integers")
    f.check_lines()
    f.gather()
    exact('dgrad', f.dgrad(d['prev']['dgrad']), want['dgrad'], "integers")
    with tuning_env(GHM_BLCONV_NO_WT='1'):
        exact('dgrad', f.dgrad(d['prev']['dgrad']), want['dgrad'], "integers, the packed weights read as they lie")
    exact('wgrad', f.wgrad(d['prev']['wgrad']), want['wgrad'], "integers")
    f.settle((R.row_id(row), "integer pass"))


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_id)
def test_reals(gpu, mem, row):
    d = cached(('real', row.g), lambda: R.real_inputs(row.g))
    refs = references(row, d, 'rref')
    f = Frame(gpu, row, d)
    splits = gpu[1].blconv_frame_splits(*row.g)
    for kind, call in zip(R.KINDS, (f.fwd, f.dgrad, f.wgrad)):
        r, m, p = refs[kind]
        prev = d['prev'][kind]
        assert (p != 0).all()                                               # no signed zero decides fl32(previous + increment)
        got = call(prev)
        note(kind, got, r + p, m + np.abs(p.astype(np.float64)), "reals", k=R.bound(kind, row.g, splits[R.KINDS.index(kind)]))
        exact(kind, call(prev), got, "reals, repeated call")
        inc = call(np.zeros_like(prev))
        exact(kind, got, (p + inc).astype(np.float32), "reals, result == fl32(previous + increment)")
        if kind == 'fwd':
            f.check_lines()
            f.gather()
    f.settle((R.row_id(row), "real pass"))


def test_every_split_path_was_reached(gpu):
    """(after the rows) on a device whose CU count plans the rows onto fewer paths, this fails"""
    assert R.COVERAGE <= REACHED, sorted(R.COVERAGE - REACHED, key=str)
