"""The sequential restatements of the hydrology (tests/hydrology_ref.py) against each other, against what the
kernels run restated in numpy, and against hand-made planes whose answers are known.  No device."""
import numpy as np
import pytest

from tests import hydrology_ref as R


@pytest.fixture(scope="module")
def results():
    return [(R.terrain(H, W, q, seed), R.analyse(R.terrain(H, W, q, seed))) for H, W, q, seed in R.CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_invariants(h, r):
    H, W = h.shape
    out = R.is_outlet(H, W)
    F, D = r.filled, r.flat
    assert (F >= h).all() and np.array_equal(F[out], h[out])
    assert np.array_equal(bits(R.fill(F)), bits(F))                       # filling a filled surface changes nothing
    assert np.array_equal(bits(r.depth), bits(F - R.canonical(h))) and (r.depth >= 0).all()
    assert (D < R.SENTINEL).all() and (D >= 0).all()
    assert ((r.direction >= 0) == ~out).all() and (r.direction <= 7).all()
    rec = R.receivers(r.direction).ravel()
    live = rec >= 0
    f, d = F.ravel(), D.ravel().astype(np.int64)
    lower = (f[rec[live]] < f[live]) | ((f[rec[live]] == f[live]) & (d[rec[live]] < d[live]))
    assert lower.all()                                                     # receivers strictly decrease (F, D): a forest
    A = r.accumulation.astype(np.int64)
    assert (A >= 1).all() and A[out].sum() == H * W
    donors = np.bincount(rec[live], weights=A.ravel()[live], minlength=H * W).astype(np.int64)
    assert np.array_equal(A.ravel(), 1 + donors)                           # every cell: itself and its donors
    b = r.basin.ravel()
    assert out.ravel()[b].all() and np.array_equal(b[out.ravel()], np.nonzero(out.ravel())[0])
    assert np.array_equal(b[live], b[rec[live]])                           # constant along every receiver chain


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_invariants_and_the_relaxations_against_the_sequential_forms(results, case):
    h, r = results[case]
    check_invariants(h, r)
    F, fill_sweeps = R.relax_fill(h)
    D, flat_sweeps = R.relax_flats(r.filled)
    A, B, rounds = R.doubling(r.direction)
    assert np.array_equal(bits(F), bits(r.filled)) and np.array_equal(D, r.flat)
    assert np.array_equal(A, r.accumulation) and np.array_equal(B, r.basin)
    n = h.size
    assert fill_sweeps <= n and flat_sweeps <= n and rounds <= int(np.ceil(np.log2(n)))
    print("case %d: %d fill sweeps, %d flat sweeps, %d rounds, %d lake cells, %d non-draining cells"
          % (case, fill_sweeps, flat_sweeps, rounds, int((r.depth > 0).sum()), int((r.flat > 0).sum())))


def test_the_direction_rule_on_a_slope_with_ties():
    # a plane falling to the east: every inner cell sees E, NE and SE lower; E's slope 1 beats the diagonals' 0.707
    h = np.tile(np.arange(5, 0, -1, dtype=np.float32), (5, 1))
    r = R.analyse(h)
    assert (r.direction[1:-1, 1:-1] == 2).all() and (r.depth == 0).all() and (r.flat == 0).all()
    # a cone: the four diagonal cells next to the top tie between two cardinals and take the lowest k
    i, j = np.mgrid[0:5, 0:5]
    cone = (4 - np.maximum(abs(i - 2), abs(j - 2))).astype(np.float32)
    d = R.analyse(cone).direction
    assert d[2, 2] == 0 and d[1, 1] == 0 and d[1, 3] == 0 and d[3, 1] == 4 and d[3, 3] == 2


def test_a_3_x_3_map_with_a_pit():
    h = np.array([[5, 4, 6], [7, 1, 8], [9, 3, 5]], np.float32)
    r = R.analyse(h)
    assert r.filled[1, 1] == 3 and r.depth[1, 1] == 2 and r.flat[1, 1] == 1 and (r.flat[R.is_outlet(3, 3)] == 0).all()
    assert r.direction[1, 1] == 4                      # the one neighbour of equal F with D = 0 is S
    assert r.accumulation[2, 1] == 2 and r.accumulation.sum() == 10 and r.basin[1, 1] == 2 * 3 + 1
    check_invariants(h, r)


def test_a_bowl_with_one_notch():
    n = 9
    i, j = np.mgrid[0:n, 0:n]
    ring = np.maximum(abs(i - 4), abs(j - 4))
    h = np.where(ring == 4, 0.0, np.where(ring == 3, 10.0, ring.astype(np.float64))).astype(np.float32)   # a rim of 10
    h[4, 7] = 6.0                                      # the notch in the rim, on the east side
    r = R.analyse(h)
    inside = ring <= 2
    assert (r.filled[inside] == 6).all() and np.array_equal(r.depth[inside], 6 - h[inside])
    assert r.accumulation[4, 7] == inside.sum() + 1    # the whole bowl arrives at the notch
    assert (r.basin[inside] == 4 * n + 8).all() and r.basin[4, 7] == 4 * n + 8
    check_invariants(h, r)


def test_a_constant_plane_has_the_chessboard_distance_to_the_edge():
    H, W = 9, 12
    r = R.analyse(np.full((H, W), 0.5, np.float32))
    i, j = np.mgrid[0:H, 0:W]
    assert np.array_equal(r.flat, np.minimum(np.minimum(i, H - 1 - i), np.minimum(j, W - 1 - j)))
    assert (r.depth == 0).all()
    check_invariants(np.full((H, W), 0.5, np.float32), r)


def test_two_pits_that_merge():
    h = np.full((5, 11), 9.0, np.float32)              # one row of wall on either side, which drains outwards
    h[0, :] = h[-1, :] = h[:, 0] = h[:, -1] = 0.0
    h[2, 2:9] = 5.0                                    # a trough inside the wall ...
    h[2, 3], h[2, 7] = 1.0, 2.0                        # ... with two pits
    h[2, 5] = 6.0                                      # and a saddle between them, above the trough's floor
    h[2, 9] = 7.0                                      # the spill through the wall, above the saddle
    r = R.analyse(h)
    assert (r.filled[2, 2:9] == 7).all()               # one lake over both pits and the saddle
    assert np.array_equal(r.flat[2, 2:10], np.arange(7, -1, -1))
    assert r.accumulation[2, 9] == 8 and (r.basin[2, 2:10] == 2 * 11 + 10).all()
    check_invariants(h, r)


def test_the_hand_made_device_planes():
    s = R.serpentine()
    r = R.analyse(s)
    _, sweeps = R.relax_fill(s)
    assert sweeps > 10 * max(s.shape) and r.flat.max() > 10 * max(s.shape)     # the level travels the channel's length
    check_invariants(s, r)
    p = R.corner_pits(32, 3)
    rp = R.analyse(p)
    assert p.shape == (98, 98) and (rp.depth[31:33, 31:33] > 0).all() and (rp.depth[63:65, 63:65] > 0).all()
    check_invariants(p, rp)


def test_the_paint_restatement():
    depth = np.zeros((6, 7), np.float32)
    depth[2, 2] = 0.5
    A = np.ones((6, 7), np.uint32)
    A[5, 6] = 100
    wet0 = R.wet_mask(depth, A, 100, 0, 0.1)
    assert wet0.sum() == 2 and wet0[2, 2] and wet0[5, 6]
    wet2 = R.wet_mask(depth, A, 100, 2, 0.1)
    assert wet2.sum() == 1 + 9 and wet2[3:, 4:].all()
    t = np.full((1, 6, 7), 0.25, np.float32)
    out = R.paint_planes(t, wet0, (0.75,), 0.5)
    assert out[0, 2, 2] == 0.5 and out[0, 0, 0] == 0.25
