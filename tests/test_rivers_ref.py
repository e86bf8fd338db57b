"""tests/rivers_ref.py against itself and against what is known of its cases: the walk by the definition, the
ranking by literal doubling, the orders.  The few counts asserted here keep a case from silently going trivial.  No device."""
import numpy as np
import pytest

import gan_heightmaps_amd.rivers as RV      # noqa: F401  (the module these restatements belong to)
from tests import rivers_ref as R


def reaches(e):
    return [e["vertex"][e["offsets"][r]:e["offsets"][r + 1]].tolist() for r in range(e["reaches"])]


def test_single_row_column():
    e = R.expected("single")
    assert (e["cells"], e["reaches"], e["isolated"], e["mouths"], e["sources"], e["rounds"]) == (1, 0, 1, 1, 1, 0)
    assert e["kind"].tolist() == [[R.STREAM | R.SOURCE | R.MOUTH]]
    assert len(e["vertex"]) == 0 and e["offsets"].tolist() == [0] and len(e["downstream"]) == 0 and len(e["order"]) == 0
    e = R.expected("row")
    assert reaches(e) == [list(range(9))] and e["downstream"].tolist() == [-1] and e["area"].tolist() == [9]
    assert (e["order"].tolist(), e["magnitude"].tolist(), e["main"].tolist()) == ([1], [1], [1])
    assert e["kind"][0, 8] == R.STREAM | R.MOUTH | 1 << 4 and e["rounds"] == 3 and e["max_rank"] == 8
    c = R.expected("column")
    assert reaches(c) == [list(range(9))] and np.array_equal(c["kind"].T, e["kind"])


def test_stars():
    e = R.expected("star")
    assert e["reaches"] == 8 and e["isolated"] == 0 and e["confluences"] == 1 and e["mouths"] == 1 and e["rounds"] == 0
    assert reaches(e) == [[c, 4] for c in (0, 1, 2, 3, 5, 6, 7, 8)] and (e["downstream"] == -1).all()
    assert e["kind"][1, 1] == R.STREAM | R.CONFLUENCE | R.MOUTH | 8 << 4 and (e["area"] == 1).all() and (e["main"] == 1).all()
    e = R.expected("star_t9")
    assert (e["cells"], e["reaches"], e["isolated"]) == (1, 0, 1) and int(e["kind"][1, 1]) == R.STREAM | R.SOURCE | R.MOUTH
    e = R.expected("star7")
    assert e["reaches"] == 8 and e["isolated"] == 2 and e["kind"][1, 1] == R.STREAM | R.CONFLUENCE | 7 << 4
    trunk = int(np.flatnonzero(e["downstream"] == -1)[0])
    assert reaches(e)[trunk] == [4, 7, 10] and e["order"][trunk] == 2 and e["magnitude"][trunk] == 7 and e["area"][trunk] == 10
    others = [r for r in range(8) if r != trunk]
    assert all(e["downstream"][r] == trunk and e["order"][r] == 1 for r in others)
    assert [int(e["main"][r]) for r in others] == [1, 0, 0, 0, 0, 0, 0]          # equal areas: the lowest reach number


def test_comb_and_empty():
    e = R.expected("comb")
    W = 600
    assert e["reaches"] == 2 * W + W - 1 and e["cells"] == 3 * W and e["isolated"] == 0
    assert (np.diff(e["offsets"]) == 2).all() and e["rounds"] == 0
    assert ((e["kind"][1] >> 4) == 3).sum() == W - 1 and e["kind"][1, 0] >> 4 == 2          # the first trunk cell has no western donor
    assert e["order"].max() == 2 and e["magnitude"].max() == 2 * (W - 1)          # the last trunk cell is a mouth: it starts no reach
    e = R.expected("empty")
    assert e["cells"] == 0 and e["reaches"] == 0 and not e["kind"].any()


def test_serpentine():
    e = R.expected("serpentine_t8")
    assert e["reaches"] == 1 and len(e["vertex"]) == 506 and e["rounds"] == 9
    e = R.expected("serpentine_t200")
    assert e["reaches"] == 1 and len(e["vertex"]) == 434


def test_noise_keeps_its_hard_cells():
    e = R.expected("noise0_t1")
    d, A, T = R.planes("noise0_t1")
    assert d.shape == (96, 80) and e["cells"] == 96 * 80
    both = R.CONFLUENCE | R.MOUTH
    assert e["reaches"] == 3063 and e["isolated"] == 246 and int(((e["kind"] & both) == both).sum()) == 17
    assert int(((e["kind"] >> 4) >= 3).sum()) == 375 and int(e["order"].max()) == 6


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_answer_hangs_together(name):
    e = R.expected(name)
    d, A, T = R.planes(name)
    H, W = d.shape
    off, v, down = e["offsets"], e["vertex"], e["downstream"]
    assert off[0] == 0 and off[-1] == len(v) and (np.diff(off) >= 2).all() and len(down) == e["reaches"]
    flat = e["kind"].ravel()
    seen = np.zeros(H * W, int)
    for r in range(e["reaches"]):
        line = v[off[r]:off[r + 1]]
        assert (flat[line] & R.STREAM).all()
        for a, b in zip(line[:-1], line[1:]):
            assert R.receiver(d, a // W, a % W) == (b // W, b % W)
        assert not (flat[line[1:-1]] & (R.CONFLUENCE | R.MOUTH)).any()
        seen[line[:-1]] += 1
        if down[r] >= 0:
            assert v[off[down[r]]] == line[-1] and e["order"][down[r]] >= e["order"][r]          # orders never fall downstream
        else:
            assert flat[line[-1]] & R.MOUTH
            if flat[line[-1]] >> 4 == 1:
                seen[line[-1]] += 1
    # every stream cell but the isolated ones and the confluence-mouths is the vertex of its own of exactly one reach
    ends = (flat & R.MOUTH != 0) & ((flat & R.SOURCE != 0) | (flat & R.CONFLUENCE != 0))
    assert np.array_equal(seen, ((flat & R.STREAM != 0) & ~ends).astype(int))
    assert e["sources"] - e["isolated"] == int((e["magnitude"][down == -1]).sum()) if e["reaches"] else True
    for m in np.flatnonzero((flat & R.MOUTH != 0) & (flat & R.CONFLUENCE != 0)):
        assert int(e["main"][(down == -1) & (v[off[1:] - 1] == m)].sum()) == (flat[m] >> 4)
    for c in set(down[down >= 0].tolist()):
        assert int(e["main"][down == c].sum()) == 1


def test_refusals_of_the_definition():
    d, A, T = R.planes("row")
    for at, v, match in (((0, 3), 9, "direction"), ((0, 3), -2, "direction"), ((0, 8), 2, "outside"), ((0, 0), 6, "outside")):
        bad = d.copy()
        bad[at] = v
        with pytest.raises(ValueError, match=match):
            R.definition(bad, A, T)
    bad = A.copy()
    bad[0, 5] = 5
    with pytest.raises(ValueError, match="accumulation"):
        R.definition(d, bad, T)
    R.definition(d, bad, 6)                 # the cell is no stream cell then
