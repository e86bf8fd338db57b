"""The restatement of the earthworks (tests/earthworks_ref.py) against a per-cell double loop on tiny planes, and the
properties the definition promises: the tie rule, the reach's edge, untouched and core cells, the modes, channels that never
rise downstream, road targets that do not depend on the order of the paths.  No device."""
import numpy as np
import pytest

from tests import earthworks_ref as E
from tests import hydrology_ref as HR
from tests import route_ref as RR


def brute_nearest(marks, R, threshold):
    """per cell: every marked cell of the plane, the least (d2, i, j) within the window and the disc"""
    H, W = marks.shape
    near, dist2 = np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in range(W):
            best = None
            for i in range(H):
                for j in range(W):
                    d2 = (i - y) ** 2 + (j - x) ** 2
                    if marks[i, j] >= threshold and abs(i - y) <= R and abs(j - x) <= R and d2 <= R * R:
                        best = min(best, (d2, i, j)) if best else (d2, i, j)
            if best:
                near[y, x], dist2[y, x] = best[1] * W + best[2], best[0]
    return near, dist2


@pytest.mark.parametrize("kind", E.KINDS)
def test_the_nearest_mark_equals_a_double_loop_on_tiny_planes(kind):
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 10), (12, 11)):
        for R in (0, 1, 3, 32):
            m, thr = E.marks_case(kind, H, W)
            near, dist2 = E.nearest(m, R, thr)
            bn, bd = brute_nearest(m, R, thr)
            assert np.array_equal(near, bn) and np.array_equal(dist2, bd), (kind, H, W, R)
            assert near.dtype == np.int32 and dist2.dtype == np.int32


def test_the_tie_rule_and_the_edge_of_the_reach():
    m = np.zeros((9, 9), np.uint32)
    m[4, 2] = m[4, 6] = m[2, 4] = m[6, 4] = 1                 # four marks at distance 2 of the centre
    near, dist2 = E.nearest(m, 2)
    assert near[4, 4] == 2 * 9 + 4 and dist2[4, 4] == 4        # the upper one; then the left one
    m[2, 4] = 0
    assert E.nearest(m, 2)[0][4, 4] == 4 * 9 + 2
    assert E.ties(m, 2, 1, E.nearest(m, 2)[1]) > 0
    # a mark at exactly distance R is found, one at (R, 1) is not: it lies in the window and outside the disc
    R = 5
    m = np.zeros((8, 8), np.uint32)
    m[0, R] = 1
    near, dist2 = E.nearest(m, R)
    assert near[0, 0] == R and dist2[0, 0] == R * R
    m = np.zeros((8, 8), np.uint32)
    m[1, R] = 1
    near, dist2 = E.nearest(m, R)
    assert near[0, 0] == -1 and dist2[0, 0] == -1 and near[1, 0] == W8(1, R)


def W8(i, j):
    return i * 8 + j


def test_the_table_of_a_profile():
    t = E.table(1.0, 6.0)
    assert t.shape == (37, 2) and t.dtype == np.float32
    assert (t[:2] == [0, 1]).all() and t[36, 1] == 0 and t[36, 0] == 1          # the core takes the target; at the reach: nothing
    assert (np.diff(t[:, 1]) <= 0).all() and ((t[:, 0] >= 0) & (t[:, 0] <= 1)).all()
    t = E.table(2.0, 2.5)                                                        # R = 2: the reach's fraction still shapes the blend
    assert t.shape == (5, 2) and t[4, 1] == 1 and E.table(1.5, 2.5)[4, 1] == np.float32(1 - 0.25 * 2)
    t = E.table(2.0, 2.0)                                                        # core = reach: a step
    assert (t[:, 1] == 1).all() and (t[:, 0] == 0).all()
    t = E.table(1.0, 1.0)
    assert t.tolist() == [[0, 1], [0, 1]]
    assert E.table(0.0, 0.0).tolist() == [[0, 1]]                                # reach 0: the marked cells alone


@pytest.mark.parametrize("mode", E.MODES)
def test_the_shaping_equals_a_double_loop_and_keeps_its_promises(mode):
    H, W, core, reach = 14, 17, 1.0, 4.5
    h, m, thr, target = E.shape_case((H, W), 4, 5)
    m = m.copy()
    m[3, 4] = m[10, 12] = 0xFFFFFFFF
    target[3, 4], target[10, 12] = np.float32(2.0), np.float32(-2.0)
    assert np.isnan(target).any()
    out, near, dist2 = E.carve(h, m, target, core, reach, mode, thr)
    tab = E.table(core, reach)
    for y in range(H):
        for x in range(W):
            want = h[y, x]
            if near[y, x] >= 0 and tab[dist2[y, x], 1] != 0:
                t = target.reshape(-1)[near[y, x]]
                v = np.float32(np.float32(tab[dist2[y, x], 0] * h[y, x]) + np.float32(tab[dist2[y, x], 1] * t))
                want = v if mode == 'both' else min(h[y, x], v) if mode == 'cut' else max(h[y, x], v)
            assert out[y, x].tobytes() == np.float32(want).tobytes(), (y, x)
    untouched = (near < 0) | (tab[np.maximum(dist2, 0), 1] == 0)
    assert untouched.any() and out[untouched].tobytes() == h[untouched].tobytes()            # the same bits
    core_cells = (near >= 0) & (dist2 <= 1)
    if mode == 'both':
        assert core_cells.sum() >= 2 and out[core_cells].tobytes() == target.reshape(-1)[near[core_cells]].tobytes()
        assert (out > h).any() and (out < h).any()
    if mode == 'cut':
        assert (out <= h).all() and (out < h).any() and out[10, 12] == -2 and out[3, 4] == h[3, 4]
    if mode == 'fill':
        assert (out >= h).all() and (out > h).any() and out[3, 4] == 2 and out[10, 12] == h[10, 12]


def test_channel_targets_never_rise_along_a_river():
    H, W, q, seed = HR.CASES[1]
    r = HR.analyse(HR.terrain(H, W, q, seed))
    thr, lake = 40, 1.0 / 64
    marks, target = E.channel_targets(r.filled, r.depth, r.accumulation, thr, lake)
    on = marks != 0
    assert on.any() and (r.depth > lake).any() and not (on & (r.depth > lake)).any()      # rivers and lakes; lakes stay flat
    assert np.isnan(target[~on]).all() and np.isfinite(target[on]).all() and (target[on] < r.filled[on]).all()
    links = deeper = 0
    for y, x in np.argwhere(on):
        k = int(r.direction[y, x])
        if k < 0:
            continue
        yy, xx = y + HR.OFFSETS[k][0], x + HR.OFFSETS[k][1]
        if on[yy, xx]:                                             # a chain of consecutive marked river cells
            links += 1
            assert target[yy, xx] <= target[y, x]                  # filled does not rise, the area and the depth do not fall,
            deeper += target[yy, xx] < target[y, x]                # and rounding is monotone
    assert links > 20 and deeper > 0
    big = np.array([[thr, 2 * thr - 1, 2 * thr, 1 << 31, 0xFFFFFFFF]], np.uint32)
    _, t = E.channel_targets(np.zeros((1, 5), np.float32), np.zeros((1, 5), np.float32), big, thr, lake, 0.5, 0.25, 3.0, 64.0)
    assert t.tolist() == [[-0.5 / 64, -0.5 / 64, -0.75 / 64, -3.0 / 64, -3.0 / 64]]


def test_road_targets_do_not_depend_on_the_order_of_the_paths():
    h, pen, sources = RR.case(3, 5)
    r = RR.field(h, sources, penalty=pen)
    cells = [tuple(int(v) for v in c) for c in np.argwhere(r.cost != RR.UNREACHED)[::173]]
    paths = [RR.walk(r.parent, c) for c in cells]
    assert len(paths) >= 4
    a = E.road_targets(h, r.parent, RR.raster(h.shape, paths) != 0, 8)
    b = E.road_targets(h, r.parent, RR.raster(h.shape, paths[::-1]) != 0, 8)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # a path's end alone marks its whole way home: parents of marked cells are marked
    ends = np.zeros(h.shape, bool)
    for c in cells:
        ends[c] = True
    c = E.road_targets(h, r.parent, ends, 8)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
    on = a[0] != 0
    # smooth = 0 keeps the ground; a source's window is itself; a longer window is a mean of the way ahead
    z = E.road_targets(h, r.parent, on, 0)[1]
    assert z[on].tobytes() == h[on].tobytes()
    for s in sources:
        if on[s]:
            assert a[1][s] == h[s]
    far = paths[int(np.argmax([len(p) for p in paths]))]
    assert len(far) > 9
    total = 0.0
    for y, x in far[:9]:
        total += float(h[y, x])                                    # in float64, from the cell on
    assert a[1][tuple(far[0])] == np.float32(total / 9) and np.isnan(a[1][~on]).all()
