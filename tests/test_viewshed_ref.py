"""The restatement of the viewshed (tests/viewshed_ref.py) held to itself: the double loop in Python integers against
the vectorised form, the symmetry of seeing, known answers, and that every random case the other tests use holds both classes --
seen and hidden -- in numbers: a case that is all one class tests nothing.  No device."""
import numpy as np
import pytest

from gan_heightmaps_amd import viewshed as VS
from tests import viewshed_ref as V


def test_the_constants_are_the_packages_and_the_headers():
    import os
    assert (VS.BLOCK, VS.MAX_OBSERVERS) == (V.BLOCK, V.MAX_OBSERVERS)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ghm.h")).read()
    for name, v in (("BLOCK", V.BLOCK), ("CHUNK", V.CHUNK), ("MAX_OBSERVERS", V.MAX_OBSERVERS)):
        assert "#define GHM_VIEWSHED_%s %d\n" % (name, v) in text
    assert V.CHUNK >= 32 and V.MAX_OBSERVERS > 2 * V.CHUNK                 # a mask's observers go in one launch; "many300" takes three


def test_quantise_is_one_float32_product_rounded_half_to_even():
    h = np.array([[0.0, 1.0, 0.5, 1.0 / 512, 3.0 / 512, 0.1]], np.float32)
    assert V.quantise(h, 1.0).tolist() == [[0, 256, 128, 0, 2, 26]]         # 0.5 -> 0 and 1.5 -> 2: half to even
    assert V.quantise(h, 65536.0).max() == 1 << 24
    s = np.float32(64.0 * 256.0)
    assert V.quantise(h, 64.0)[0, 5] == int(np.rint(np.float32(np.float32(0.1) * s)))
    assert V.quantise(h, 64.0).dtype == np.int32
    assert VS.quantum(2.0) == 512 and VS.quantum(0.5 / 256) == 0 and VS.quantum(1.5 / 256) == 2 and VS.quantum(65536) == 1 << 24


@pytest.mark.parametrize("name", ("one", "small", "small0", "steep", "graze"))
def test_the_two_forms_agree(name):
    c = V.case(name)
    count, mask = V.expected(name)
    lcount, lmask = V.viewshed_loop(c["zq"], c["observers"], c["target_q"])
    assert np.array_equal(count, lcount) and np.array_equal(mask, lmask)
    assert count.dtype == np.uint32 and mask.dtype == np.uint32
    bits = sum(((mask >> np.uint32(i)) & 1).astype(np.uint32) for i in range(len(c["observers"])))
    assert np.array_equal(bits, count)


def test_the_two_forms_agree_on_lines_and_beyond_32_observers():
    for name in ("row", "column"):
        c = V.case(name)
        count, mask = V.expected(name)
        lcount, lmask = V.viewshed_loop(c["zq"], c["observers"], c["target_q"])
        assert np.array_equal(count, lcount) and np.array_equal(mask, lmask)
    c = V.case("many33")
    count, mask = V.expected("many33")
    assert mask is None and count.max() <= 33
    lcount, lmask = V.viewshed_loop(c["zq"][:12, :20], [o for o in c["observers"] if o[0] < 12 and o[1] < 20], c["target_q"])
    assert lcount.max() >= 1                                               # (a corner of the plane, with the observers inside it)


def test_seeing_is_symmetric_when_eye_and_target_are_level():
    zq = V.quantise(V.heights(33, 65, 3), 8.0)
    rng = np.random.RandomState(5)
    seen = hidden = 0
    for q in (0, 384):
        for _ in range(200):
            a, b = (int(rng.randint(33)), int(rng.randint(65))), (int(rng.randint(33)), int(rng.randint(65)))
            ab = V.sees(zq, a + (q, -1), q, *b)
            assert ab == V.sees(zq, b + (q, -1), q, *a), (a, b, q)
            seen, hidden = seen + ab, hidden + (not ab)
    assert seen >= 50 and hidden >= 50
    # and a sight line reads only the bounding box of its ends: garbage outside it changes nothing
    a, b = (5, 9), (20, 40)
    wild = zq.copy()
    box = np.zeros(zq.shape, bool)
    box[5:21, 9:41] = True
    wild[~box] = 1 << 24
    for r in range(5, 21):
        for c in range(9, 41):
            assert V.sees(zq, a + (256, -1), 0, r, c) == V.sees(wild, a + (256, -1), 0, r, c)


def test_known_answers():
    flat = np.full((20, 31), 777, np.int32)
    count, mask = V.viewshed(flat, [(7, 11, 0, -1), (0, 0, 0, -1), (19, 30, 0, -1)], 0)
    assert (count == 3).all() and (mask == 7).all()                                      # every step grazes
    rr, cc = np.mgrid[0:20, 0:31]
    ramp = (40 * rr + 17 * cc).astype(np.int32)
    assert (V.viewshed(ramp, [(7, 11, 0, -1), (19, 0, 0, -1)], 0)[0] == 2).all()         # a constant ramp: every step grazes too
    assert (V.viewshed(ramp, [(7, 11, 5, -1)], 3)[0] == 1).all()
    # one wall cell hides exactly the wedge behind it: the cells whose sight line has a sample that touches the wall with weight > 0
    wall = np.zeros((21, 21), np.int32)
    wall[10, 13] = 1000
    vis = V.visible_from(wall, (10, 10, 0, -1), 0)
    want = np.ones((21, 21), bool)
    for r in range(21):
        for c in range(21):
            dy, dx = r - 10, c - 10
            n, m = max(abs(dy), abs(dx)), min(abs(dy), abs(dx))
            for k in range(1, n):
                q, f = divmod(k * m, n)
                sy, sx = (dy > 0) - (dy < 0), (dx > 0) - (dx < 0)
                pa = (10 + sy * k, 10 + sx * q) if abs(dy) >= abs(dx) else (10 + sy * q, 10 + sx * k)
                pb = (pa[0], pa[1] + sx) if abs(dy) >= abs(dx) else (pa[0] + sy, pa[1])
                if pa == (10, 13) or (f > 0 and pb == (10, 13)):
                    want[r, c] = False
    assert np.array_equal(vis, want) and want[10, 13] and not want[10, 14:].any() and want[:, :13].all()
    # (at the far edge, n = 10: the sample of step 3 lies 3 |dy| / 10 rows off the wall's row and touches it while that is < 1)
    assert (~want).sum() == 31 and not want[7:14, 20].any() and want[6, 20] and want[14, 20]
    # a radius cuts a disc
    disc = V.visible_from(flat, (7, 11, 0, 30), 0)
    assert np.array_equal(disc, (rr - 7) ** 2 + (cc - 11) ** 2 <= 30) and disc.sum() == 97
    assert V.visible_from(flat, (7, 11, 0, 0), 0).sum() == 1 and V.visible_from(flat, (7, 11, 0, 1), 0).sum() == 5
    # the equality case: the target 20 cells along sees the wall's top exactly on its line; nearer ones, behind the wall, do not
    c = V.case("graze")
    count, mask = V.expected("graze")
    row = mask[2]
    assert row[23] == 1 and (row[14:23] == 0).all() and (row[24:] == 3).all() and (row[:14] == 3).all()
    assert (np.delete(mask, 2, axis=0) == 3)[:, :13].all()
    # 32-bit products would overflow
    count, mask = V.expected("row4096")
    assert (mask[0, 3::2] == 1).all() and (mask[0, 2::2] == 0).all() and mask[0, 0] == 3 and mask[0, 1] == 3
    assert int(V.case("row4096")["zq"].max()) * 4095 > 1 << 31


def test_every_random_case_holds_both_classes():
    names = [n for n in V.CASES if V.case(n)["random"]]
    assert len(names) >= 9
    for name in names:
        c = V.case(name)
        free = [o for o in c["observers"] if o[3] < 0]
        assert free, name
        best = (0, 0)
        for o in free:
            v, f = V.visible_from(c["zq"], o, c["target_q"]), V.far(c["zq"].shape, o)
            best = max(best, (min(int(v[f].sum()), int((~v)[f].sum())), 0))
        # at least one observer without a radius sees >= 16 and misses >= 16 of the cells a sight line has a step to
        assert best[0] >= 16, (name, best)
        count, _ = V.expected(name)
        assert (count > 0).sum() >= 16 and (count < len(c["observers"])).sum() >= 16, name
    # the degenerate plane has no such cell at all
    assert not V.far((1, 1), (0, 0)).any()
