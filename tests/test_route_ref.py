"""The sequential restatements of the route module (tests/route_ref.py) against each other and against answers known
by hand: a heap Dijkstra on Python integers, the Jacobi relaxation the plain kernel runs, scipy's Dijkstra on the integer graph,
the symmetry of the weights, the parents' forest, the traffic's sum.  No device."""
import numpy as np
import pytest

from gan_heightmaps_amd import route as RT
from tests import route_ref as R

COUNTS = (1, 5)


@pytest.fixture(scope="module")
def cases():
    out = []
    for n in range(len(R.TERRAINS)):
        for count in COUNTS:
            h, pen, src = R.case(n, count)
            out.append((h, pen, src, R.field(h, src, penalty=pen)))
    for shape in ((1, 1), (1, 7), (33, 65)):
        h = R.terrain(shape[0], shape[1], None, 77)
        pen = R.sprinkled(shape[0], shape[1], 78) if shape[0] > 1 else np.ones(shape, np.float32)
        src = R.pick_sources(pen, min(2, h.size), 79)
        out.append((h, pen, src, R.field(h, src, penalty=pen)))
    return out


def test_the_module_and_the_restatement_state_the_same_constants():
    assert (RT.UNIT, RT.MAX_WEIGHT, RT.UNREACHED, RT.NO_PARENT) == (R.UNIT, R.MAX_WEIGHT, R.UNREACHED, R.NO_PARENT) == \
        (64, 1 << 24, 0xFFFFFFFF, -2)
    assert RT.OFFSETS == R.OFFSETS and RT.KEEP == ('cost', 'parent', 'territory', 'traffic')
    t = RT.Travel()
    assert tuple(getattr(t, k) for k in R.Travel._fields) == tuple(R.TRAVEL)


def test_dijkstra_equals_jacobi_on_every_case(cases):
    counts = []
    for h, pen, src, r in cases:
        cj, sweeps = R.jacobi(r.q, src)
        assert cj.dtype == np.uint32 and np.array_equal(cj, r.cost)
        assert 1 <= sweeps <= h.size
        counts.append(sweeps)
        reached = r.cost != R.UNREACHED
        assert reached[tuple(zip(*src))].all() and (r.cost[tuple(zip(*src))] == 0).all()
        assert not reached[~np.isfinite(pen)].any() or all(~np.isfinite(pen[s]) for s in src)
    print("jacobi sweeps %s" % counts)
    assert max(counts) > 32                             # the shared cases need more sweeps than one tile's inner cap


def test_both_agree_with_scipy_on_the_integer_graph(cases):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    for h, pen, src, r in cases:
        H, W = h.shape
        rows, cols, vals = [], [], []
        idx = np.arange(H * W).reshape(H, W)
        for k, (dy, dx) in enumerate(R.OFFSETS):
            m = r.q[k] != 0
            rows.append(idx[m])
            cols.append(idx[m] + dy * W + dx)
            vals.append(r.q[k][m].astype(np.float64))       # integers below 2^24: sums below 2^53 are exact in float64
        if not sum(len(v) for v in vals):
            assert h.size == 1
            continue
        g = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
        d = dijkstra(g, directed=True, indices=R.flat_sources(src, W), min_only=True)
        want = np.where(np.isfinite(d) & (d < R.UNREACHED), d, R.UNREACHED).astype(np.uint64).astype(np.uint32).reshape(H, W)
        assert np.array_equal(want, r.cost)


def test_the_weights_are_symmetric_positive_and_below_the_clamp(cases):
    for h, pen, src, r in cases:
        H, W = h.shape
        for k, (dy, dx) in enumerate(R.OFFSETS):
            ya, xa = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yb, xb = slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx))
            assert np.array_equal(r.q[k][ya, xa], r.q[(k + 4) % 8][yb, xb]), k
            edge = np.ones((H, W), bool)
            edge[ya, xa] = False
            assert (r.q[k][edge] == 0).all()           # an edge that leaves the plane
        assert r.q.max() <= R.MAX_WEIGHT
        blocked = ~np.isfinite(pen)
        assert (r.q[:, blocked] == 0).all()
        if h.size > 1:
            assert r.q.max() >= R.UNIT


def test_parents_descend_in_cost_and_reach_a_source(cases):
    for h, pen, src, r in cases:
        reached = r.cost != R.UNREACHED
        assert ((r.parent == R.NO_PARENT) == ~reached).all()
        assert ((r.parent == -1) == (r.cost == 0)).all() and int((r.parent == -1).sum()) == len(set(src))
        assert (r.parent[reached & (r.cost != 0)] >= 0).all()          # every reached cell finds a parent
        for i, j in np.argwhere(reached)[::7]:
            p = R.walk(r.parent, (i, j))
            c = r.cost[p[:, 0], p[:, 1]].astype(np.int64)
            assert (np.diff(c) < 0).all() and c[-1] == 0 and tuple(p[-1]) in set(src)
            assert r.territory[i, j] == min(n for n, s in enumerate(src) if s == tuple(p[-1]))


def test_traffic_over_the_sources_counts_the_reached_cells(cases):
    for h, pen, src, r in cases:
        reached = r.cost != R.UNREACHED
        roots = sorted(set(src))
        assert int(r.traffic[tuple(zip(*roots))].astype(np.int64).sum()) == int(reached.sum())
        assert (r.traffic[~reached] == 0).all() and (r.traffic[reached] >= 1).all()
        assert (r.territory[~reached] == -1).all() and (r.territory[reached] >= 0).all()
        for n in np.unique(r.territory[reached]):
            assert int((r.territory == n).sum()) == int(r.traffic[src[n]])


def test_a_flat_strip_costs_64_a_step_and_a_diagonal_91():
    r = R.field(np.zeros((1, 9), np.float32), [(0, 0)])
    assert np.array_equal(r.cost[0], 64 * np.arange(9)) and np.array_equal(r.parent[0], [-1] + [6] * 8)
    assert np.array_equal(r.traffic[0], np.arange(9, 0, -1))
    r = R.field(np.full((6, 6), 0.25, np.float32), [(0, 0)])
    assert r.q[3, 0, 0] == 91 == int(np.rint(np.float32(1.41421356) * 64)) and r.q[2, 0, 0] == 64
    i, j = np.mgrid[0:6, 0:6]
    assert np.array_equal(r.cost, 91 * np.minimum(i, j) + 64 * np.abs(i - j))
    assert r.parent[3, 3] == 7 and r.parent[0, 3] == 6 and r.parent[3, 0] == 0
    assert r.parent[2, 1] == 0                          # N then NW and NW then N cost the same: the lowest k


def test_a_slope_costs_what_the_definition_says():
    h = np.array([[0.0, 1.0 / 64]], np.float32)        # one cell of rise over one cell of run with height_scale 64
    q = R.weights(h, R.TRAVEL._replace(grade=1.0))
    assert q[2, 0, 0] == q[6, 0, 1] == 128             # a step at the grade costs twice its flat cost
    q = R.weights(h, R.TRAVEL._replace(grade=0.5))
    assert q[2, 0, 0] == 64 * 5                        # 1 + (1 / 0.5)^2


def test_a_wall_with_one_gap():
    h = np.zeros((9, 11), np.float32)
    pen = np.ones((9, 11), np.float32)
    pen[:, 5] = np.inf
    pen[7, 5] = 1                                       # the gap
    r = R.field(h, [(1, 1)], penalty=pen)
    assert (r.cost[:7, 5] == R.UNREACHED).all() and r.cost[8, 5] == R.UNREACHED and r.cost[7, 5] != R.UNREACHED
    # to (1, 9): diagonally down to the gap's row would overshoot; the way is 4 columns to the gap's door with 6 rows of descent
    assert r.cost[7, 5] == 4 * 91 + 2 * 64 and r.cost[1, 9] == r.cost[7, 5] + 4 * 91 + 2 * 64
    p = R.walk(r.parent, (1, 9))
    assert (7, 5) in {tuple(c) for c in p} and tuple(p[-1]) == (1, 1)
    sealed = R.field(h, [(1, 1)], penalty=np.where(np.arange(11)[None, :] == 5, np.inf, pen).astype(np.float32))
    assert (sealed.cost[:, 5:] == R.UNREACHED).all() and (sealed.territory[:, 6:] == -1).all()


def test_the_adversarial_planes_are_what_their_names_say():
    h, pen, src, end, units = R.serpentine()
    assert h.shape == (67, 67)
    r = R.field(h, [src], penalty=pen)
    assert int(r.cost[end]) == units == int(r.cost[np.isfinite(pen)].max()) and units > 30 * 64 * 67
    _, sweeps = R.jacobi(r.q, [src])
    assert sweeps > 30 * 67                             # the corridor, cell by cell
    h, pen, at = R.walled_in()
    r = R.field(h, [at], penalty=pen)
    assert int((r.cost != R.UNREACHED).sum()) == 1 and r.parent[at] == -1 and r.traffic[at] == 1 and r.territory[at] == 0
    assert (np.delete(r.parent.ravel(), at[0] * h.shape[1] + at[1]) == R.NO_PARENT).all()
    # a source on an impassable cell reaches itself alone
    pen = np.ones((5, 6), np.float32)
    pen[2, 3] = np.inf
    r = R.field(np.zeros((5, 6), np.float32), [(2, 3)], penalty=pen)
    assert int((r.cost != R.UNREACHED).sum()) == 1 and r.cost[2, 3] == 0
    # a lake that cannot be crossed is walked around
    h, depth = R.lake_plane()
    travel = R.TRAVEL._replace(lake=np.inf)
    r = R.field(h, [(18, 2)], travel, depth=depth)
    dry = R.field(h, [(18, 2)], travel)
    assert (r.cost[depth > 0] == R.UNREACHED).all() and (r.cost[depth == 0] != R.UNREACHED).all()
    assert r.cost[18, 37] > dry.cost[18, 37] == 35 * 64
    wet = R.field(h, [(18, 2)], R.TRAVEL, depth=depth)                   # lake = 16: crossing costs, the shore costs half of it
    assert dry.cost[18, 37] < wet.cost[18, 37] <= r.cost[18, 37]


def test_two_sources_at_equal_cost_break_the_tie_by_the_lowest_k():
    h = np.zeros((5, 9), np.float32)
    r = R.field(h, [(2, 0), (2, 8)])
    assert (r.cost[:, 4] == r.cost[2, 4]).sum() >= 1 and r.cost[2, 4] == 4 * 64
    assert r.parent[2, 4] == 2 and r.territory[2, 4] == 1              # E (k = 2) before W (k = 6)
    assert r.parent[2, 3] == 6 and r.parent[2, 5] == 2
    same = R.field(h, [(2, 0), (2, 0), (2, 8)])                          # duplicates keep the lowest ordinal
    assert set(np.unique(same.territory)) == {0, 2}


def test_saturation_every_edge_clamps_and_the_strip_ends_at_the_255th_cell():
    h, pen, src = R.saturated_strip()
    r = R.field(h, [src], penalty=pen)
    assert (r.q[2, 0, :-1] == R.MAX_WEIGHT).all()
    assert np.array_equal(r.cost[0, :256].astype(np.int64), np.arange(256, dtype=np.int64) << 24)
    assert (r.cost[0, 256:] == R.UNREACHED).all() and (r.parent[0, 256:] == R.NO_PARENT).all()
    assert r.traffic[0, 0] == 256
    cj, _ = R.jacobi(r.q, [src])
    assert np.array_equal(cj, r.cost)


def test_jacobi_resumes_from_a_finished_field_that_gains_a_source():
    h, pen, src = R.case(3, 5)
    q = R.weights(h, penalty=pen)
    first, _ = R.jacobi(q, src[:4])
    again, sweeps = R.jacobi(q, src[:4], start=first)
    assert sweeps == 1 and np.array_equal(again, first)
    more, _ = R.jacobi(q, src, start=first)
    assert np.array_equal(more, R.dijkstra(q, src)) and not np.array_equal(more, first)


def test_the_hosts_grouping_rule():
    assert R.host_sweeps(1, 1) == 1                    # one cell: one sweep, which changes nothing
    assert R.host_sweeps(7, 7) == 7                    # a strip of 7: six sweeps that change, the seventh alone
    assert R.host_sweeps(2, 4) == 4                    # 2 x 2: three sweeps, then the fourth alone
    assert R.host_sweeps(1, 10000) == 8 and R.host_sweeps(8, 10000) == 16 and R.host_sweeps(9, 10000) == 16
    assert R.host_sweeps(10, 10000) == 24


def test_the_raster_marks_the_cells_of_the_paths():
    m = R.raster((4, 5), [np.array([[0, 0], [1, 1]]), np.array([[3, 4]])])
    assert m.dtype == np.uint32 and m.sum() == 3 and m[0, 0] == m[1, 1] == m[3, 4] == 1
    assert np.array_equal(RT.raster((4, 5), [np.array([[10, 20], [11, 21]]), np.array([[13, 24]])], origin=(10, 20)), m)
