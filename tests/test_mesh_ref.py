"""The two numpy restatements of the adaptive mesh (tests/mesh_ref.py) against each other, and the properties
the mesh is built for: manifold, exact area, one winding, exact at tolerance 0, two triangles per tile at tolerance 1, fewer
triangles at larger tolerances, errors that depend on T - 2 pixels outside a tile and no more, rectangles that stitch.  No GPU."""
import numpy as np
import pytest

from tests import mesh_ref as M

FORESTS = ((1, 1), (2, 3), (3, 3))
TOLS = (0.0, 0.004, 0.02, 0.1, 1.0)


def _plane(k, R, C):
    T = 1 << k
    return M.case(10 * k + R + C, R * T + 1, C * T + 1, k)


@pytest.mark.parametrize("k", (1, 2, 3, 4))
@pytest.mark.parametrize("forest", FORESTS)
def test_the_recursion_and_the_gather_give_the_same_errors(k, forest):
    h, e = _plane(k, *forest)
    assert e.dtype == np.float32 and M.errors_recursive(h, k).tobytes() == e.tobytes()
    assert M.errors_scalar(h, k).tobytes() == e.tobytes()
    T = 1 << k
    assert np.isinf(e[::T, ::T]).all() and np.isfinite(e).sum() == e.size - (forest[0] + 1) * (forest[1] + 1)


@pytest.mark.parametrize("k", (1, 2, 3, 4))
@pytest.mark.parametrize("forest", FORESTS)
def test_the_descent_and_the_predicate_give_the_same_mesh(k, forest):
    h, e = _plane(k, *forest)
    T, (R, C) = 1 << k, forest
    rect = (0, 0, R * T, C * T)
    last = None
    for tol in TOLS:
        grid, heights, tris = M.extract(h, e, k, tol)
        pts = M.as_points(grid, tris)
        rec = np.asarray(M.triangles_recursive(e, k, np.float32(tol)))
        assert M.multiset(pts) == M.multiset(rec)
        assert M.bad_edges(pts, rect) == 0
        cr = M.crosses(pts)
        assert (cr > 0).all() and cr.sum() == 2 * R * C * T * T        # one winding; the areas sum to the rectangle
        assert np.array_equal(heights, h[grid[:, 0], grid[:, 1]]) and np.array_equal(grid, np.argwhere(e > np.float32(tol)))
        assert last is None or len(tris) <= last                       # F does not grow with the tolerance
        last = len(tris)
        if tol == 1.0:
            assert len(tris) == 2 * R * C and len(grid) == (R + 1) * (C + 1)
        if tol == 0.0:
            assert np.array_equal(M.surface(pts, heights[tris.astype(np.int64)], h.shape).astype(np.float32), h)


@pytest.mark.parametrize("k", (2, 3, 4))
def test_errors_reach_T_minus_2_pixels_outside_a_tile_and_no_further(k):
    T = 1 << k
    h, e = _plane(k, 3, 3)
    rng = np.random.RandomState(k)

    def inner_after_changing_outside(margin):
        g = h.copy()
        m = np.ones(h.shape, bool)
        m[T - margin:2 * T + margin + 1, T - margin:2 * T + margin + 1] = False
        g[m] = rng.rand(int(m.sum())).astype(np.float32)
        return M.errors(g, k)[T:2 * T + 1, T:2 * T + 1]
    inner = e[T:2 * T + 1, T:2 * T + 1]
    assert np.array_equal(inner_after_changing_outside(T), inner)                  # one ring of tiles is enough
    assert np.array_equal(inner_after_changing_outside(T - 2), inner)              # ... and so are T - 2 pixels
    assert not np.array_equal(inner_after_changing_outside(T - 3), inner)          # ... and not one fewer
    if T > 4:
        bad = np.argwhere(inner_after_changing_outside(T // 2) != inner)
        assert len(bad) and set(bad.ravel().tolist()) <= {0, T // 2, T}            # the tile's mid-edge vertices feel it
    # the mesh of the inner tile follows its errors
    g = h.copy()
    g[:1], g[-1:], g[:, :1], g[:, -1:] = 0.0, 1.0, 0.5, 0.25
    e2 = M.errors(g, k)
    rect = (T, T, T, T)
    for a, b in zip(M.extract(h, e, k, 0.02, rect), M.extract(g, e2, k, 0.02, rect)):
        assert np.array_equal(a, b)


def _world_mesh(rect, k, tol):
    """the mesh of a tile-aligned rectangle of the unbounded function: errors over the rectangle grown by a ring of tiles,
    extraction on the inner tiles -> triangles as absolute points, heights per corner"""
    T = 1 << k
    y0, x0, hh, ww = rect
    g = M.world_heights(y0 - T, x0 - T, hh + 2 * T, ww + 2 * T)
    grid, heights, tris = M.extract(g, M.errors(g, k), k, tol, (T, T, hh, ww))
    return M.as_points(grid, tris, (y0, x0)), heights[tris.astype(np.int64)]


@pytest.mark.parametrize("k", (2, 3))
def test_rectangles_of_an_unbounded_world_stitch(k):
    T, tol = 1 << k, 0.03
    whole = (-2 * T, T, 2 * T, 3 * T)
    left, right = (-2 * T, T, 2 * T, T), (-2 * T, 2 * T, 2 * T, 2 * T)
    pw, vw = _world_mesh(whole, k, tol)
    parts = [_world_mesh(r, k, tol) for r in (left, right)]
    for (p, v), r in zip(parts, (left, right)):
        inside = ((pw[:, :, 0] >= r[0]) & (pw[:, :, 0] <= r[0] + r[2]) & (pw[:, :, 1] >= r[1]) &
                  (pw[:, :, 1] <= r[1] + r[3])).all(1)
        assert np.array_equal(p, pw[inside]) and np.array_equal(v, vw[inside])      # the restriction, in the same order
    union = np.concatenate([p for p, _ in parts])
    assert M.multiset(union) == M.multiset(pw) and M.bad_edges(union, whole) == 0
    assert 2 * 6 < len(pw) < 2 * 6 * T * T                                           # neither trivial nor full
    # without the ring the two do not fit: the border's errors miss what lies beyond it
    g = M.world_heights(*left)
    lonely = M.errors(g, k)
    ringed = M.world_heights(left[0] - T, left[1] - T, left[2] + 2 * T, left[3] + 2 * T)
    assert not np.array_equal(lonely[:, -1], M.errors(ringed, k)[T:-T, -T - 1])
