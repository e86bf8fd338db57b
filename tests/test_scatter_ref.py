"""The restatement of the scatter (tests/scatter_ref.py) against itself: sort-and-greedy equals the Jacobi fixed point of
the local rule, both hold the two invariants of a Poisson-disk thinning, which are checked without either; the mixer is a fair
coin, its streams differ and negative world coordinates are places of their own; the chance's table lookups.  No device."""
import numpy as np
import pytest

from tests import scatter_ref as S


@pytest.mark.parametrize("kind", S.KINDS)
def test_greedy_equals_the_jacobi_fixed_point(kind):
    for shape in ((1, 1), (1, 40), (33, 65), (70, 45)):
        for s2 in (1, 2, 3, 16, 50, 1024):
            state, prio = S.thin_case(kind, shape)
            want = S.thin(state, prio, s2)
            got, sweeps = S.jacobi(state, prio, s2, max_sweeps=shape[0] * shape[1] + 1)
            assert np.array_equal(got, want), (kind, shape, s2)
            assert S.invariants(state, prio, s2, want) is None, (kind, shape, s2)
            if s2 == 1:
                assert np.array_equal(want == S.KEPT, state == 1) and sweeps <= 2          # every candidate is kept
            if kind == 'random' and shape == (70, 45) and s2 > 1:
                assert 2 < sweeps < 40 and 0 < (want == S.KEPT).sum() < (want == S.REJECTED).sum()


def test_ties_go_to_the_row_then_the_column():
    state, prio = S.thin_case('equal', (9, 9))
    state[:] = 1
    out = S.thin(state, prio, 2)
    assert out[0, 0] == S.KEPT and out[0, 1] == S.REJECTED and out[1, 0] == S.REJECTED and out[1, 1] == S.KEPT
    assert np.array_equal(S.jacobi(state, prio, 2)[0], out)
    assert np.array_equal(S.points(out)[:3], [[0, 0], [0, 2], [0, 4]])


@pytest.mark.parametrize("rising", (True, False))
def test_the_staircase_takes_one_sweep_per_cell(rising):
    for shape in ((1, 300), (300, 1)):
        state, prio = S.staircase(shape, rising)
        want = S.thin(state, prio, 2)
        got, sweeps = S.jacobi(state, prio, 2)
        assert np.array_equal(got, want) and sweeps == 301
        line = want.reshape(-1) if rising else want.reshape(-1)[::-1]
        assert (line[0::2] == S.KEPT).all() and (line[1::2] == S.REJECTED).all()
        assert S.invariants(state, prio, 2, want) is None


def test_the_invariants_catch_what_they_are_for():
    state, prio = S.thin_case('random', (20, 30))
    out = S.thin(state, prio, 16)
    assert S.invariants(state, prio, 16, out) is None
    r, c = S.points(out)[3]
    bad = out.copy()
    bad[r, c + 1 if c + 1 < 30 else c - 1] = S.KEPT
    assert "within the spacing" in S.invariants(state, prio, 16, bad)
    bad = out.copy()
    bad[r, c] = S.REJECTED                                         # no longer maximal: somebody near has lost its excuse, or it itself
    assert "rejected candidate" in S.invariants(state, prio, 16, bad)
    bad = out.copy()
    bad[r, c] = S.UNDECIDED
    assert "candidates" in S.invariants(state, prio, 16, bad)
    none = np.zeros_like(state)
    assert "candidates" in S.invariants(none, prio, 16, out)


def test_the_mixer_is_a_fair_coin_with_streams_and_negative_coordinates():
    half = np.full((128, 128), 1 << 23, np.uint32)
    for seed, origin in ((0, (0, 0)), (1, (0, 0)), (0xDEADBEEFCAFEF00D, (-64, -64)), (7, (-1000000, 12345)), (-3, (5, -5))):
        state, prio = S.candidates(half, seed, origin)
        assert abs(int(state.sum()) - 8192) <= 320, (seed, origin, int(state.sum()))        # five standard deviations
        assert abs(int((prio >> np.uint32(31)).sum()) - 8192) <= 320
        assert np.unique(prio).size > 16384 - 40                                            # 2^14 draws of 2^32: ~0.03 collisions
    assert S.candidates(np.full((4, 4), S.ONE, np.uint32), 3)[0].all()                     # chance 2^24: always
    assert not S.candidates(np.zeros((4, 4), np.uint32), 3)[0].any()                       # chance 0: never
    r, c = np.mgrid[-8:8, -8:8]
    a, b = S.hash32(5, 0, r, c), S.hash32(5, 1, r, c)
    assert (a != b).mean() > 0.99 and np.unique(a).size == a.size                          # the streams differ
    assert (S.hash32(5, 0, -r, c) != a)[r != 0].all() and (S.hash32(5, 0, r, -c) != a)[c != 0].all()
    assert (S.hash32(5, 0, c, r) != a)[r != c].all()                                       # (row, col) is not (col, row)
    assert (S.hash32(5, 0, r, c) != S.hash32(5 + (1 << 32), 0, r, c)).all()                 # the seed's high word counts
    assert np.array_equal(S.hash32(5, 0, r - (1 << 32), c), a)                              # coordinates are taken modulo 2^32
    assert int(S.hash32(0, 0, 0, 0)) != 0
    # a window of the world is the world's: candidates and priorities are functions of the world position
    big = S.candidates(half, 11, (-70, -20))
    part = S.candidates(half[:50, :60], 11, (-40, 10))
    assert np.array_equal(big[0][30:80, 30:90], part[0]) and np.array_equal(big[1][30:80, 30:90], part[1])


def test_the_chance_and_its_tables():
    b = S.slope_bounds()
    assert b.dtype == np.float32 and b.size == 63 and (np.diff(b) > 0).all() and b[31] == np.float32(1.0)     # 45 degrees
    ones = S.tables(np.ones(256), np.ones(64))
    flat = np.full((5, 6), 0.5, np.float32)
    assert (S.chance(flat, ones, 64, 1.0) == S.ONE).all() and (S.chance(flat, ones, 64, 0.25) == S.ONE // 4).all()
    assert (S.chance(flat, ones, 64, 0.0) == 0).all()
    alt = np.zeros(256)
    alt[128] = 1.0                                                  # 0.5 * 255 + 0.5 = 128
    only = S.tables(alt, np.ones(64))
    assert (S.chance(flat, only, 64, 1.0) == S.ONE).all() and (S.chance(flat + np.float32(0.01), only, 64, 1.0) == 0).all()
    wild = np.array([[-3.0, 7.0, 1e30, -1e30]], np.float32)          # heights outside [0, 1] clamp to the table's ends
    alt = np.zeros(256)
    alt[0], alt[255] = 0.5, 1.0
    got = S.chance(wild, S.tables(alt, np.ones(64)), 1e-30, 1.0)
    assert got.tolist() == [[S.ONE // 2, S.ONE, S.ONE, S.ONE // 2]]
    ramp = (np.arange(8, dtype=np.float32) / np.float32(64))[None, :].repeat(3, 0)          # slope 1 inside: 45 degrees, bin 32
    slope = np.zeros(64)
    slope[32] = 1.0
    got = S.chance(ramp, S.tables(np.ones(256), slope), 64, 1.0)
    assert (got[:, 1:-1] == S.ONE).all() and (got[:, 0] == 0).all()                         # the edge sees half the difference
    water = np.array([0.0, 1.0, 0.5, 0.25], np.float32)                                     # d2 = 0, 1, 2, and everything else
    d2 = np.array([[0, 1, 2, 3, -1, 99]], np.int32)
    got = S.chance(flat[:1], ones, 64, 1.0, d2, water)
    assert got.tolist() == [[0, S.ONE, S.ONE // 2, S.ONE // 4, S.ONE // 4, S.ONE // 4]]
    blocked = np.array([[0, 1, 2, 3, 4, 5]], np.uint32)
    assert S.chance(flat[:1], ones, 64, 1.0, blocked=blocked, threshold=3).tolist() == [[S.ONE] * 3 + [0] * 3]
