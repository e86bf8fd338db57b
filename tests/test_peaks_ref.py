"""The peaks' reference against itself (tests/peaks_ref.py): the definition -- a descending union-find over the cells --
and what the device does -- ascent, labels, the regions' maximum spanning tree, the grouped merge -- agree on every case; the
invariants; the small cases' answers worked out by hand.  No device."""
import numpy as np
import pytest

from tests import peaks_ref as R


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_two_routes_agree_and_the_invariants_hold(name):
    e = R.expected(name)
    zq = e["zq"]
    H, W = zq.shape
    d = R.definition(zq)
    for k in ("summit", "col", "parent", "prominence_q"):
        assert d[k].dtype == e[k].dtype and np.array_equal(d[k], e[k]), k
    # Kruskal and Boruvka mark the same edges: the weights are unique
    assert np.array_equal(R.kruskal(zq, e["label"]), e["tree"])
    P = len(e["summit"])
    assert e["tree"].shape == (P - 1, 3) and P >= 1
    assert int(e["summit_area"].sum()) == H * W
    z = zq.ravel().astype(np.int64)
    assert (e["prominence_q"] <= z[e["summit"]] - z.min()).all() and (e["prominence_q"] >= 0).all()
    assert (e["parent"] == -1).sum() == 1 and (e["col"] == -1).sum() == 1
    # a parent's prominence is no less and its key is greater, so the reported peaks' parents stand before them
    for min_q, top in ((1, None), (3, None), (1, 5)):
        keep, parent = R.report(e["summit"], z[e["summit"]], e["col"], e["parent"], e["prominence_q"], min_q, top)
        assert all(p < i for i, p in enumerate(parent)) and (e["prominence_q"][keep] >= min_q).all()
        assert all(parent[i] >= 0 or e["parent"][keep[i]] == -1 for i in range(len(keep)))
        if top is not None:
            assert len(keep) <= top
    # every cell climbs to its label by cells of ever greater key
    asc, label = e["ascent"].ravel(), e["label"].ravel()
    for i in range(H * W):
        if asc[i] >= 0:
            n = (i // W + R.DY[asc[i]]) * W + i % W + R.DX[asc[i]]
            assert (z[n], n) > (z[i], i) and label[n] == label[i]
        else:
            assert label[i] == i


def test_the_small_cases_by_hand():
    e = R.expected("single")
    assert e["summit"].tolist() == [0] and e["prominence_q"].tolist() == [0] and e["rounds"] == 0 and e["tree"].shape == (0, 3)
    e = R.expected("row")                                                   # 3 1 4 1 5 9 2 6 5
    assert e["summit"].tolist() == [0, 2, 5, 7]
    assert e["col"].tolist() == [1, 3, -1, 6] and e["parent"].tolist() == [2, 2, -1, 2] and e["prominence_q"].tolist() == [2, 3, 8, 4]
    e = R.expected("column")                                                # 2 7 1 8 2 8 1: of the two 8 the later is the higher
    assert e["summit"].tolist() == [1, 3, 5] and e["col"].tolist() == [2, 4, -1] and e["parent"].tolist() == [2, 2, -1]
    assert e["prominence_q"].tolist() == [6, 6, 7]
    e = R.expected("flat")
    assert e["summit"].tolist() == [29] and e["prominence_q"].tolist() == [0] and e["summit_area"].tolist() == [30]
    assert len(R.report(e["summit"], [77], e["col"], e["parent"], e["prominence_q"])[0]) == 0
    e = R.expected("two_peaks")
    assert e["summit"].tolist() == [8, 12] and e["col"].tolist() == [-1, 10] and e["parent"].tolist() == [-1, 0]
    assert e["prominence_q"].tolist() == [9, 4] and e["rounds"] == 1
    e = R.expected("triple")                                                # both losers die at the centre, the 9 their parent
    assert e["summit"].tolist() == [0, 2, 7] and e["col"].tolist() == [-1, 4, 4] and e["parent"].tolist() == [-1, 0, 0]
    assert e["prominence_q"].tolist() == [9, 3, 2] and e["tree"][:, 0].tolist() == [4, 4]
    e = R.expected("lambda")                                                # two summits on one plateau: prominence 0
    assert e["summit"].tolist() == [3, 5] and e["col"].tolist() == [1, -1] and e["prominence_q"].tolist() == [0, 4]
    z = e["zq"].ravel()
    keep, parent = R.report(e["summit"], z[e["summit"]], e["col"], e["parent"], e["prominence_q"])
    assert keep.tolist() == [1] and parent.tolist() == [-1]
    e = R.expected("extremes")
    assert e["prominence_q"].max() == 1 << 25


def test_the_cases_stress_what_they_are_named_for():
    e = R.expected("ruler")
    assert len(e["summit"]) == 64 and e["rounds"] == 6
    assert e["prominence_q"].max() == 1063 - 450                            # the highest peak over the lowest saddle
    e = R.expected("staircase")
    assert len(e["summit"]) == 128 and e["rounds"] == 1
    assert e["parent"].tolist() == [127] * 127 + [-1]
    # every peak picks the saddle towards the next one: the one round's hooks form a chain of 127
    assert sorted(map(sorted, e["tree"][:, 1:].tolist())) == [[2 * i, 2 * i + 2] for i in range(127)]
    e = R.expected("spiral")
    assert len(e["summit"]) == 1 and e["hops"] > 1024                       # the label doubling needs at least 11 rounds
    e = R.expected("noise37")
    assert len(np.unique(e["zq"])) == 6 and (e["prominence_q"] == 0).any()
    assert len(R.expected("noise96")["summit"]) > 8 and len(R.expected("blocks")["summit"]) > 8
