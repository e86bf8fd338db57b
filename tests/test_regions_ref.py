"""The regions' reference (tests/regions_ref.py) agrees with itself: the components against a second labelling, the successor is a
permutation, the two outer / hole properties of include/ghm.h, section "regions", 4., and the counts of the cases.  No device.

The longest hole.  The value noise of the contour tests is smooth -- lattice values eight cells apart, bilinear between them -- and
on 96 x 131 cells no seed in 0 .. 149 and no level (one level from 6000 to 10500 in steps of 250; bands of 512 .. 8192) gives a
hole ring of more than 632 edges, so ``bands96`` cannot hold one of more than 1024.  That property -- a hole whose ranking needs
more than ten rounds -- is asserted on ``moat`` instead, whose one hole is the serpentine's ring of 1224 edges; ``bands96`` keeps
what it is there for: tile borders crossed, holes inside holes, and an outer ring of more than 2048 edges (rounds = 12)."""
import numpy as np
import pytest

from tests import regions_ref as R


def relabel(L):
    """the components once more, by repeated min over equal-label 4-neighbours"""
    H, W = L.shape
    comp = np.where(L >= 0, np.arange(H * W).reshape(H, W), -1).astype(np.int64)
    while True:
        new = comp.copy()
        for a, b in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:])):
            m = (L[a] == L[b]) & (L[a] >= 0)
            new[a] = np.where(m, np.minimum(new[a], comp[b]), new[a])
        if np.array_equal(new, comp):
            return comp.astype(np.int32)
        comp = new


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_reference_agrees_with_itself(name):
    L, e = R.case(name), R.expected(name)
    H, W = L.shape
    assert np.array_equal(e["component"], relabel(L))
    assert (e["component"] <= np.arange(H * W).reshape(H, W)).all() and ((e["component"] >= 0) == (L >= 0)).all()
    P, Rn, E = e["polygons"], e["rings"], e["edges"]
    assert e["seed"].tolist() == sorted(e["seed"].tolist()) and np.array_equal(e["component"].ravel()[e["seed"]], e["seed"])
    assert e["cells"].sum() == (L >= 0).sum() and np.array_equal(e["polygon"].ravel()[e["seed"]], np.arange(P))
    assert np.array_equal(e["label"], L.ravel()[e["seed"]])
    # the successor is a permutation, and its cycles are the rings
    assert sorted(e["succ"].tolist()) == list(range(E)) and e["ring_edges"].sum() == E
    assert E == sum(int(R.is_edge(L, r, c, s)) for r in range(H) for c in range(W) for s in range(4))
    # exactly one outer ring per polygon, of positive area; every hole negative; the doubled areas sum to 2 cells
    area2 = R.doubled_areas(e, W)
    outer = e["ring_hole"] == 0
    assert np.array_equal(np.sort(e["ring_polygon"][outer]), np.arange(P))
    assert (area2[outer] > 0).all() and (area2[~outer] < 0).all()
    assert np.array_equal(np.bincount(e["ring_polygon"], weights=area2, minlength=P).astype(np.int64), 2 * e["cells"].astype(np.int64))
    # vertices turn: no collinear corner, every step along one axis, every ring closed with at least four of them
    for k in range(Rn):
        v = e["vertex"][e["ring_offsets"][k]:e["ring_offsets"][k + 1]].astype(np.int64)
        d = np.stack([np.roll(v, -1) // (W + 1) - v // (W + 1), np.roll(v, -1) % (W + 1) - v % (W + 1)], 1)
        assert len(v) >= 4 and len(v) % 2 == 0 and ((d != 0).sum(1) == 1).all()
        assert ((d[:, 0] != 0) != (np.roll(d, -1, axis=0)[:, 0] != 0)).all()
        assert np.abs(d).sum() == e["ring_edges"][k]
    assert e["ring_offsets"][0] == 0 and e["ring_offsets"][-1] == e["vertices"] == len(e["vertex"]) and e["holes"] == Rn - P


def test_the_counts_of_the_table():
    for name, want in R.TABLE.items():
        e = R.expected(name)
        assert (e["edges"], e["rings"], e["polygons"], e["holes"], e["vertices"]) == want, name
    assert int(R.expected("serpentine")["cells"][0]) == 611 and R.expected("serpentine")["rounds"] == 11
    # one label, two polygons; a hole ring through one corner twice; regions kept apart at a corner
    assert R.expected("diag")["label"].tolist() == [0, 0]
    e = R.expected("hole_pinch")
    hole = e["vertex"][e["ring_offsets"][1]:e["ring_offsets"][2]].tolist()
    assert e["ring_hole"].tolist() == [0, 1, 0, 0] and hole.count(2 * 5 + 2) == 2 and len(hole) == 8
    assert R.expected("pinch")["cells"].tolist() == [4, 4]
    # labels are compared, never used as indices
    a, b = R.expected("nested"), R.expected("nested_7_max")
    assert b["label"].tolist() == [7, 2 ** 31 - 1, 7] and all(np.array_equal(a[k], b[k]) for k in ("vertex", "ring_polygon", "ring_hole", "cells"))
    e = R.expected("empty")
    assert (e["edges"], e["rings"], e["polygons"], e["vertices"], e["rounds"]) == (0, 0, 0, 0, 0) and e["ring_offsets"].tolist() == [0]
    assert R.expected("row")["polygons"] == 6 and R.expected("column")["polygons"] == 10


def test_the_noise_planes_cross_tiles_with_holes_inside_holes():
    for name in ("land37", "bands37", "land96", "bands96"):
        e = R.expected(name)
        assert e["holes"] >= 1 and max(R.case(name).shape) > 32, name
    e, L = R.expected("bands96"), R.case("bands96")
    # a hole inside a hole: a polygon that lies in a hole of a polygon that itself lies in a hole
    inside = {}                                                            # polygon -> the polygon whose hole holds it
    for k in np.flatnonzero(e["ring_hole"]):
        v = int(e["vertex"][e["ring_offsets"][k]])                         # of the cells round a hole's corner, those of other polygons lie in it
        r, c = v // (L.shape[1] + 1), v % (L.shape[1] + 1)
        for q in set(e["polygon"][r - 1:r + 1, c - 1:c + 1].ravel().tolist()) - {int(e["ring_polygon"][k])}:
            inside.setdefault(int(q), int(e["ring_polygon"][k]))
    assert any(inside.get(inside[p]) is not None for p in inside)
    assert e["rounds"] == 12 and e["ring_edges"].max() > 2048
    # the hole whose ranking needs more than ten rounds (see the module's docstring)
    m = R.expected("moat")
    assert m["ring_hole"].tolist() == [0, 1, 0] and m["ring_edges"][1] == 1224 > 1024 and m["rounds"] == 11
