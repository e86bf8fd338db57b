"""The sunlight's restatement (tests/sunlight_ref.py) against itself, without a device: its two forms agree; the early
exit and the block-maximum jumps, restated, change nothing; a window grown by the reach reproduces the larger plane and a smaller
one does not; the energy on a tilted plane is the float64 cosine within the quantisation's own bound; the cases hold what they are
for."""
import math

import numpy as np
import pytest

from tests import sunlight_ref as R


def test_the_table_holds_every_kind_of_position():
    t = R.table(R.ALL_SUNS)
    assert t.shape == (18, R.FIELDS) and ((t[:, 3] == 0) == (t[:, 2] == 0)).all()
    axes = t[8:16]
    assert axes[::2, 3].tolist() == [0] * 4 and axes[1::2, 3].tolist() == [R.ONE] * 4                # m_q = 0 and m_q = 65536
    assert {(int(p[0]), int(p[1]), int(p[2])) for p in axes} == {(1, 1, 0), (1, 1, 1), (0, 1, 0), (0, 1, -1), (1, -1, 0), (1, -1, -1),
                                                                   (0, -1, 0), (0, -1, 1)}             # every octant's edge
    assert {(int(p[0]), int(p[1]), int(p[2])) for p in t[:8] if p[3] not in (0, R.ONE)} >= {(1, -1, -1), (1, 1, 1), (0, -1, 1), (0, 1, 1)}
    assert t[16, 4] == R.MAX_RISE and t[16, 5:8].tolist() == [0, 0, 16384]                            # an elevation of 90 degrees
    assert t[17, 4] == 1 and t[17, 7] == 0                                                            # rise_q clamps to 1
    assert (t[:, 3] >= 0).all() and (t[:, 3] <= R.ONE).all() and (t[:, 4] >= 1).all() and t[:, 8].sum() <= R.MAX_WEIGHT
    wall = R.case("wall")["table"]
    assert wall[0, 4] == 4096 and wall[0, :4].tolist() == [0, 1, 0, 0] and wall[2, 1] == -1
    assert R.position(0, 30)[4] == int(np.rint(65536 * math.tan(math.radians(30))))
    for name in ("many33", "many300"):
        assert R.case(name)["table"][:, 8].sum() <= R.MAX_WEIGHT
    assert len(R.case("many33")["table"]) == 33 and len(R.case("many300")["table"]) > 4 * R.CHUNK


@pytest.mark.parametrize("name", ["1x1", "1x9", "9x1", "15x17", "17x33", "wall"])
def test_the_loop_and_the_vectorised_form_agree(name):
    c = R.case(name)
    assert R.same_planes(R.sunlight_loop(c["zq"], c["table"], c["target_q"]), R.expected(name)), name


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_early_exit_changes_nothing(name):
    want, early = R.expected(name), R.expected_early(name)
    assert R.same_planes(want, early), name
    assert (early["steps"] <= want["steps"]).all()
    if name in ("65x130", "row4096"):
        assert early["steps"].sum() < want["steps"].sum()                   # and it does end rays early


def test_the_cases_hold_both_outcomes():
    for name in ("33x65", "37x70", "70x37", "65x130"):
        c, e = R.case(name), R.expected(name)
        for i in range(16):                                                 # the prototype's suns and the eight axes
            on = (e["mask"] >> np.uint32(i)) & 1
            assert 0 < on.sum(), (name, i)
            if R.ALL_SUNS[i][1] <= 28:                                      # the high suns (45 and 80 degrees) may light every cell
                assert on.sum() < on.size, (name, i)
        assert R.expected_steps(name).max() > 100, name
    e = R.expected("wall")
    at = R.WALL_AT - R.WALL_STEPS
    assert e["mask"][1, at] & 1 == 1 and e["mask"][3, at] & 1 == 0         # grazing is lit; one unit of zq more shades
    assert e["mask"][1, at + 1] & 1 == 0 and e["mask"][3, at - 1] & 1 == 1
    c = R.case("row4096")
    assert int(c["zq"].max()) == 1 << 24 and c["table"][1, 4] == 1 and c["table"][2, 4] == R.MAX_RISE
    e = R.expected("row4096")
    assert not np.array_equal(e["lit"][0, 0:4094:2], e["lit"][0, 1:4095:2]) and len(np.unique(e["lit"])) >= 2      # low and high cells differ
    assert R.expected("many33")["mask"] is None and R.expected("33x65")["mask"] is not None


@pytest.mark.parametrize("name", ["1x9", "9x1", "15x17", "17x33", "wall"])
def test_block_maximum_jumps_change_nothing(name):
    c = R.case(name)
    zq, tops = c["zq"], R.top(c["zq"])
    gy, gx, _ = R.slope(zq)
    plain_total = accel_total = 0
    for p in c["table"]:
        dot = -gy * int(p[5]) - gx * int(p[6]) + 512 * int(p[7])
        want, steps = R.lit_plane(zq, p, c["target_q"], dot > 0, early=True)
        for r, col in zip(*np.nonzero(dot > 0)):
            lit, tested = R.lit_accel(zq, tops, p, c["target_q"], int(r), int(col))
            assert lit == want[r, col] and tested <= steps[r, col], (name, p.tolist(), r, col)
            plain_total += int(steps[r, col])
            accel_total += tested
    if name in ("15x17", "17x33", "wall"):
        assert accel_total < plain_total                                    # and runs are jumped


def test_a_window_grown_by_the_reach_reproduces_the_larger_plane():
    h = R.V.heights(80, 120, 51)
    scale = 4.0
    tab = R.table([(90, 8), (200, 12, 0.5), (315, 10), (10, 40)])
    reach = R.reach(tab, scale)
    assert reach == -(-256 * 1024 // int(tab[:, 4].min())) + 1 == 30
    zq = R.quantise(h, scale)
    whole = R.sunlight(zq, tab, 0)
    r0, r1, c0, c1 = 32, 48, 35, 85
    win = R.sunlight(zq[r0 - reach:r1 + reach, c0 - reach:c1 + reach], tab, 0)
    for k in R.PLANES:
        assert np.array_equal(win[k][reach:-reach, reach:-reach], whole[k][r0:r1, c0:c1]), k
    inner = whole["lit"][r0:r1, c0:c1]
    assert (inner < 4).sum() > 50 and (inner == 4).sum() > 50             # there are shadows to agree on


def test_a_smaller_window_does_not():
    """A level plane, the sun due +x, one wall of the largest height the scale allows.  The cell T has the wall D columns ahead.
    The wall blocks T's ray iff 65536 Z > 256 D rise_q, i.e. iff D <= ceil(256 Z / rise_q) - 1 = reach - 2: the farthest cell that
    can shade lies reach - 2 cells away.  So a window that ends reach - 3 cells beyond T loses the wall and lights T, and one that
    ends reach - 2 cells beyond T still holds it: the reach, reach - 2 + 1 for the cell b and + 1 for the step that clears, is safe
    with two cells to spare on this axis-aligned ray, and reach - 3 is the first margin that shows a difference."""
    scale = 4.0
    tab = R.table([(90, 20)])
    reach = R.reach(tab, scale)
    D = reach - 2
    h = np.zeros((5, 40), np.float32)
    T = (2, 8)
    h[2, T[1] + D] = 1.0
    zq = R.quantise(h, scale)
    assert int(zq.max()) == 1024 and 65536 * 1024 > 256 * D * int(tab[0, 4]) and 65536 * 1024 <= 256 * (D + 1) * int(tab[0, 4])
    whole = R.sunlight(zq, tab, 0)
    assert whole["lit"][T] == 0
    short = R.sunlight(zq[:, :T[1] + (reach - 3) + 1], tab, 0)
    assert short["lit"][T] == 1                                             # the window lost the wall
    enough = R.sunlight(zq[:, :T[1] + (reach - 2) + 1], tab, 0)
    assert enough["lit"][T] == 0
    grown = R.sunlight(zq[:, :T[1] + reach + 1], tab, 0)
    assert np.array_equal(grown["lit"][:, :T[1] + 1], whole["lit"][:, :T[1] + 1])


def test_the_energy_on_a_tilted_plane_is_the_cosine_within_the_quantisations_bound():
    """No shadows on a plane under suns well above it, so energy = sum of floor(w_q dot / norm).  Against e* = w_q 2^14 cos(angle
    between the integer normal (-g_y, -g_x, 512) and the float64 direction to the sun), with N = |normal|:
      dot = 2^14 dot* + d, |d| <= (|g_y| + |g_x| + 512) / 2 <= (sqrt(3) / 2) N      (each entry of s is rounded once, by at most 1/2)
      norm in (N - 1, N], so 0 <= 1 / norm - 1 / N < 1 / (N (N - 1))
      w dot / norm - e* = w dot (1 / norm - 1 / N) + w d / N,  |dot| <= N (2^14 + sqrt(3) / 2)
    so |e - e*| <= w_q ((2^14 + sqrt(3) / 2) / (N - 1) + sqrt(3) / 2) + 1 per position, the 1 for the floor."""
    H, W = 24, 40
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    scale = 64.0
    h = ((0.30 * rr - 0.20 * cc + 10.0) / scale).astype(np.float32)
    assert h.min() > 0 and h.max() < 1
    suns = [(0, 60, 1.0), (135, 45, 2.0), (250, 70, 0.5), (90, 35, 1.5)]
    tab = R.table(suns)
    zq = R.quantise(h, scale)
    got = R.sunlight(zq, tab, 0)
    assert (got["lit"] == len(suns)).all()
    gy, gx, _ = R.slope(zq)
    N = np.sqrt((gy * gy + gx * gx + 512 * 512).astype(np.float64))
    want, bound = np.zeros((H, W)), np.zeros((H, W))
    for (az, el, hours), p in zip(suns, tab):
        a, e = math.radians(az), math.radians(el)
        d = (math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e))
        cos = (-gy * d[0] - gx * d[1] + 512 * d[2]) / N
        assert (cos > 0.2).all()
        want += int(p[8]) * 16384.0 * cos
        bound += int(p[8]) * ((16384.0 + math.sqrt(3) / 2) / (N - 1) + math.sqrt(3) / 2) + 1
    err = np.abs(got["energy"].astype(np.float64) - want)
    assert (err <= bound).all() and bound.max() < 0.01 * want.min()
    # and against the cosine of the plane itself, away from the clamped edge: the heights' rounding moves a gradient by at most 1
    n = np.array([-0.30, 0.20, 1.0]) / math.sqrt(0.30 ** 2 + 0.20 ** 2 + 1)
    ideal = sum(int(p[8]) * 16384.0 * (n[0] * math.cos(math.radians(el)) * math.cos(math.radians(az)) +
                                       n[1] * math.cos(math.radians(el)) * math.sin(math.radians(az)) + n[2] * math.sin(math.radians(el)))
                for (az, el, _), p in zip(suns, tab))
    assert np.abs(got["energy"][1:-1, 1:-1] / ideal - 1).max() < 0.01
