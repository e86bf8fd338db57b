"""Properties of the contours' definition as tests/contour_ref.py restates it, checked on its own: every segment lies
in exactly one line, open lines run from border to border and loops close, consecutive vertices share a cell, higher ground lies
on one fixed side, every t lies strictly inside its edge; then the known answers of the sixteen corner codes, both saddle
resolutions and the tie, a single peak, a steep cell; and that ``contour.Levels`` names the levels the restatement draws.  No
device."""
from fractions import Fraction

import numpy as np
import pytest

from gan_heightmaps_amd import contour as CT
from tests import contour_ref as R

RANDOM = ("noise37", "noise37_512", "integers", "clipped", "negative_base", "serpentine", "serpentine_open")


def position(v):
    """the exact position (row, col) of a vertex whose t is the exact quotient"""
    r, c, axis, t = v
    return (Fraction(r) + (t if axis else 0), Fraction(c) + (0 if axis else t))


def exact_t(Z, v, lm):
    r, c, axis, _ = v
    a = int(Z[r, c])
    b = int(Z[r + 1, c]) if axis else int(Z[r, c + 1])
    return Fraction(lm - a, b - a)


def cells_of(v):
    r, c, axis = v[:3]
    return {(r - 1, c), (r, c)} if axis == 0 else {(r, c - 1), (r, c)}


@pytest.mark.parametrize("name", RANDOM)
def test_every_segment_lies_in_exactly_one_line_and_lines_end_on_the_border(name):
    c = R.case(name)
    H, W = c["zq"].shape
    segs = R.segments(c["zq"], c["base_q"], c["interval_q"], c["count"])
    assert [s[0] for s in segs] == sorted(s[0] for s in segs) and len({s[0] for s in segs}) == len(segs)          # the key order
    lines = R.lines_of(segs, (H, W))
    seen = sorted(i for _, ids in lines for i in ids)
    assert seen == list(range(len(segs)))
    assert [ids[0] for _, ids in lines] == sorted(ids[0] for _, ids in lines)

    def on_border(v):
        r, c_, axis = v[:3]
        return (axis == 0 and r in (0, H - 1)) or (axis == 1 and c_ in (0, W - 1))

    for closed, ids in lines:
        for a, b in zip(ids, ids[1:]):
            assert segs[a][2] == segs[b][1] and segs[a][0][2] == segs[b][0][2]          # exit vertex = entry vertex, one level
        if closed:
            assert segs[ids[-1]][2] == segs[ids[0]][1] and ids[0] == min(ids)
        else:
            assert on_border(segs[ids[0]][1]) and on_border(segs[ids[-1]][2])
    tr, _ = R.expected(name)
    assert tr["segments"] == len(segs) and len(tr["level"]) == len(lines)
    assert np.array_equal(np.diff(tr["offsets"]), [len(ids) + (0 if cl else 1) for cl, ids in lines])
    # consecutive vertices of a line share a cell
    for i in range(len(lines)):
        vs = [tuple(v) for v in tr["edge"][tr["offsets"][i]:tr["offsets"][i + 1]].tolist()]
        for a, b in zip(vs, vs[1:] + (vs[:1] if tr["closed"][i] else [])):
            if a is not b:
                assert cells_of(a) & cells_of(b)


@pytest.mark.parametrize("name", RANDOM[:5] + ("tie", "saddle_a_above", "saddle_a_below", "saddle_b_above", "saddle_b_below"))
def test_higher_ground_lies_on_one_side_and_t_inside_its_edge(name):
    c = R.case(name)
    Z = 2 * c["zq"].astype(np.int64)
    for (r, col, j, e), p, q, x in R.segments(c["zq"], c["base_q"], c["interval_q"], c["count"]):
        lm = R.lam(j, c["base_q"], c["interval_q"])
        assert 0.0 < p[3] < 1.0 and 0.0 < q[3] < 1.0 and e != x
        pp = position(p[:3] + (exact_t(Z, p, lm),))
        qq = position(q[:3] + (exact_t(Z, q, lm),))
        assert p[3] == float(exact_t(Z, p, lm)) and q[3] == float(exact_t(Z, q, lm))          # the correctly rounded quotient
        # the corners above the level at the ends of the two edges the segment crosses (at a saddle whose centre is below, the
        # far corner is above too, but behind the cell's other segment)
        ends = {R.CORNERS[k % 4] for k in (e, e + 1, x, x + 1)}
        above = [(r + dr, col + dc) for dr, dc in ends if Z[r + dr, col + dc] > lm]
        assert above and len(above) < len(ends)
        for ar, ac in above:
            # (q - p) x (a - p) > 0 with vectors written (col, row)
            cross = (qq[1] - pp[1]) * (ar - pp[0]) - (qq[0] - pp[0]) * (ac - pp[1])
            assert cross > 0, (r, col, j, e)


def test_levels_name_the_restatements_levels():
    """level j of a Levels is lam_j = 2 (base_q + j interval_q) + 1: odd, 1/512 cell above its nominal height"""
    for lv in (CT.Levels(), CT.Levels(1.5, -0.75, 4, 3), CT.Levels(1 / 256, 65536.0), CT.Levels(0.3, 0.1)):
        for j in (-7, -1, 0, 1, 5, 1000):
            lm = R.lam(j, lv.base_q, lv.interval_q)
            assert lm % 2 == 1 and Fraction(lm, 512) - Fraction(1, 512) == Fraction(lv.base_q + j * lv.interval_q, 256)
            exact = lv.interval * 256 == lv.interval_q and lv.base * 256 == lv.base_q
            assert not exact or Fraction(lm - 1, 512) == Fraction(lv.height(j))
            assert lv.is_index(j) == (j % lv.index_every == 0)
    # count keeps the levels 0 .. count - 1, whatever lies below or above
    assert list(R.level_range(-10 ** 6, 10 ** 6, 0, 256, CT.Levels(count=3).count)) == [0, 1, 2]
    # no height of the grid lies on a level: between a height and itself there is none, between neighbours in 1/256 cell at most one
    for zq in range(-5, 6):
        assert len(R.level_range(2 * zq, 2 * zq, 0, 1)) == 0 and list(R.level_range(2 * zq, 2 * zq + 2, 0, 1)) == [zq]


def test_the_sixteen_codes():
    """entry and exit edge of the one-cell plane whose corners TL, TR, BR, BL lie above level 0 where bit 3, 2, 1, 0 is set"""
    want = {0: [], 15: [],
            8: [(0, 3)], 4: [(1, 0)], 2: [(2, 1)], 1: [(3, 2)],                    # one corner above: round it
            7: [(3, 0)], 11: [(0, 1)], 13: [(1, 2)], 14: [(2, 3)],                 # one corner below
            12: [(1, 3)], 6: [(2, 0)], 3: [(3, 1)], 9: [(0, 2)],                   # a straight crossing
            10: [(0, 3), (2, 1)], 5: [(1, 0), (3, 2)]}                             # the tie: the centre counts as below
    for code in range(16):
        segs = R.segments(R.code_cell(code), 0, 1, 1)
        assert [(s[0][3], s[3]) for s in segs] == want[code], code
        assert all(s[1][3] == 0.5 and s[2][3] == 0.5 for s in segs)
        tr = R.expected("code%02d" % code)[0]
        assert len(tr["level"]) == len(want[code]) and not tr["closed"].any()


def test_both_saddle_resolutions_and_the_tie():
    def edges(name):
        c = R.case(name)
        return [(s[0][3], s[3]) for s in R.segments(c["zq"], c["base_q"], c["interval_q"], c["count"])]
    assert edges("saddle_a_above") == [(0, 1), (2, 3)]           # TL and BR above, joined: TR and BL are cut off
    assert edges("saddle_a_below") == [(0, 3), (2, 1)]           # TL and BR are cut off
    assert edges("saddle_b_above") == [(1, 2), (3, 0)]
    assert edges("saddle_b_below") == [(1, 0), (3, 2)]
    assert edges("tie") == [(1, 0), (3, 2)]
    tr = R.expected("tie")[0]                                     # two open lines of one segment each
    assert tr["offsets"].tolist() == [0, 2, 4] and tr["closed"].tolist() == [0, 0] and tr["level"].tolist() == [0, 0]
    assert tr["edge"].tolist() == [[0, 1, 1], [0, 0, 0], [0, 0, 1], [1, 0, 0]] and tr["t"].tolist() == [0.5] * 4


def test_a_single_peak_and_a_steep_cell():
    tr = R.expected("peak")[0]                                    # 0 .. 1024 at interval_q 256: four loops around the centre
    assert tr["closed"].tolist() == [1, 1, 1, 1] and np.diff(tr["offsets"]).tolist() == [4, 4, 4, 4] and tr["level"].tolist() == [0, 1, 2, 3]
    one = R.trace(R.case("peak")["zq"], 512, 256, 1)
    assert one["closed"].tolist() == [1] and one["segments"] == 4 and one["level"].tolist() == [0]
    assert one["edge"].tolist() == [[1, 0, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]]           # from the cell (0, 0), whose BR is the peak
    assert one["t"].tolist() == [1025 / 2048, 1025 / 2048, 1 - 1025 / 2048, 1 - 1025 / 2048]
    tr = R.expected("steep")[0]                                   # corners 0 and 16384: the levels 0 .. 63
    assert tr["segments"] == 64 and tr["level"].tolist() == list(range(64)) and not tr["closed"].any()
    assert R.expected("steep_diag")[0]["segments"] == 64 + 20     # 20 of its levels cross a saddle


def test_the_issues_figures():
    for name, lines, closed in (("noise37", 276, 55), ("noise96_512", 677, 393)):
        tr = R.expected(name)[0]
        assert (len(tr["level"]), int(tr["closed"].sum())) == (lines, closed), name
    tr = R.expected("serpentine")[0]
    assert tr["segments"] == 4604 and tr["closed"].tolist() == [1] and tr["longest"] == 4604
    tr = R.expected("serpentine_open")[0]
    assert tr["segments"] == 4606 and tr["closed"].tolist() == [0] and np.diff(tr["offsets"]).tolist() == [4607]
    assert R.expected("row")[0]["segments"] == 0 and R.expected("column")[0]["offsets"].tolist() == [0]


def test_count_clips_on_both_sides_and_a_negative_base():
    c = R.case("clipped")
    every = R.trace(c["zq"], c["base_q"], c["interval_q"], None)
    tr = R.expected("clipped")[0]
    assert set(tr["level"].tolist()) == set(range(6)) and every["level"].min() < 0 and every["level"].max() > 5
    assert tr["segments"] < every["segments"]
    n = R.expected("negative_base")[0]
    assert n["level"].min() > 0                                   # the base lies below the plane: level 0 is not on it


def test_the_marks():
    zq = np.array([[300, 300, 600], [300, 600, 2000]], np.int32)
    # at interval_q 256 a height of 300 lies above the levels below 2, 600 above those below 3, 2000 above those below 8:
    # 300 | 600 is parted by level 2, 600 | 2000 by the levels 3 .. 7, of which 5 is an index contour
    assert R.marks(zq, 0, 256, None, 5).tolist() == [[0, 1, 2], [1, 2, 0]]
    assert R.marks(zq, 0, 256, 1, 5).tolist() == [[0, 0, 0], [0, 0, 0]] and R.marks(zq, 400, 256, 1, 5).tolist() == [[0, 2, 0], [2, 0, 0]]
    assert R.marks(-zq, 0, 256, None, 5).tolist() == [[0, 1, 2], [1, 2, 0]]          # -600 | -300: level -2; -2000 | -600: -7 .. -3
    for name in ("noise37", "clipped", "negative_base"):
        c = R.case(name)
        mk = R.expected(name)[1]
        assert set(np.unique(mk)) == {0, 1, 2} and mk[-1, -1] == 0
        # a marked pixel is the first end of a crossed grid edge: the vertices' edges are the marks
        tr = R.expected(name)[0]
        hit = np.zeros(mk.shape, bool)
        hit[tr["edge"][:, 0], tr["edge"][:, 1]] = True
        assert np.array_equal(hit, mk > 0)
