"""The window rule of TerrainWorld.flight (gan_heightmaps_amd/world.py plan_windows / flight_plan) and the command
line's --window-mb.  No GPU."""
import math

import numpy as np
import pytest

from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd import world as WD
from tests.test_world_plan import _world


def _line(n, start, end, size=(20, 28), **kw):
    """n cameras on the straight line from start to end (y, x, z)"""
    cam = dict(yaw=0.5, pitch=-0.35, fov=1.0)
    cam.update(kw)
    return [RN.Camera(tuple(p + (q - p) * i / max(n - 1, 1) for p, q in zip(start, end)), size=size, **cam)
            for i in range(n)]


def _inside(f, rect):
    return rect[0] <= f[0] and rect[1] <= f[1] and f[0] + f[2] <= rect[0] + rect[2] and f[1] + f[3] <= rect[1] + rect[3]


def _check_plan(plan, fps, snap, cap):
    # windows cover all frames, as consecutive runs, in order
    assert plan[0][1] == 0 and plan[-1][2] == len(fps) - 1
    for (_, i, j), (_, i2, _) in zip(plan, plan[1:]):
        assert i <= j and i2 == j + 1
    for w, (rect, i, j) in enumerate(plan):
        # corners on multiples of snap (floor / ceiling: Python's % is the floor modulus), within the cap
        assert all(v % snap == 0 for v in (rect[0], rect[1], rect[0] + rect[2], rect[1] + rect[3])), rect
        assert rect[2] * rect[3] <= cap
        for k in range(i, j + 1):
            assert _inside(fps[k], rect), (k, fps[k], rect)
        # the smallest snapped rectangle around its frames, nothing more
        assert rect == WD.snap_out(RN.union_footprint(fps[i:j + 1]), snap)
        # greedy maximality: one more frame would exceed the cap
        if j + 1 < len(fps):
            grown = WD.snap_out(RN.union_footprint(fps[i:j + 2]), snap)
            assert grown[2] * grown[3] > cap, (w, grown)


def test_snap_out_floors_and_ceils():
    assert WD.snap_out((-37, 19, 101, 75), 32) == (-64, 0, 128, 96)
    assert WD.snap_out((-1, -33, 1, 1), 32) == (-32, -64, 32, 32)          # truncation would give 0 and -32
    assert WD.snap_out((-64, 32, 64, 32), 32) == (-64, 32, 64, 32)         # already there: unchanged
    assert WD.snap_out((5, -7, 3, 9), 1) == (5, -7, 3, 9)
    for y0 in range(-70, 70, 7):
        for n in (1, 31, 32, 33):
            a, _, h, _ = WD.snap_out((y0, 0, n, 1), 32)
            assert a % 32 == 0 and h % 32 == 0 and a <= y0 < y0 + n <= a + h and a > y0 - 32 and a + h < y0 + n + 32


@pytest.mark.parametrize("snap", [32, 1, 48])
def test_plan_covers_the_path_in_greedy_snapped_windows(snap):
    cams = _line(40, (-700.5, 11.25, 14.0), (700.0, -320.0, 14.0))         # crosses y = 0 and x = 0
    fps = [c.footprint(40.0) for c in cams]
    one = max(WD.snap_out(f, snap)[2] * WD.snap_out(f, snap)[3] for f in fps)
    for cap in (one, 3 * one, 10 * one):
        plan = WD.plan_windows(fps, snap, cap)
        _check_plan(plan, fps, snap, cap)
        assert WD.plan_windows(list(fps), snap, cap) == plan               # the same inputs, the same plan
    assert len(WD.plan_windows(fps, snap, 10 ** 9)) == 1


def test_a_straight_path_of_40_frames_with_room_for_about_5():
    cams = _line(40, (-400.0, 50.0, 14.0), (400.0, 50.0, 14.0), yaw=0.0)
    fps = [c.footprint(40.0) for c in cams]
    five = WD.snap_out(RN.union_footprint(fps[:5]), 32)
    cap = five[2] * five[3]
    plan = WD.plan_windows(fps, 32, cap)
    _check_plan(plan, fps, 32, cap)
    assert len(plan) >= 6
    assert plan[0][1:] == (0, plan[0][2]) and plan[0][2] >= 4               # the first window holds those five at least


def test_a_stationary_camera_needs_one_window():
    cam = RN.Camera((-20.5, 11.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28))
    fps = [cam.footprint(40.0)] * 25
    s = WD.snap_out(fps[0], 32)
    assert WD.plan_windows(fps, 32, s[2] * s[3]) == [(s, 0, 24)]
    assert WD.plan_windows([], 32, 100) == []


def test_a_single_oversize_frame_raises_and_names_the_frame():
    cams = _line(6, (-100.0, 0.0, 14.0), (100.0, 0.0, 14.0))
    fps = [c.footprint(40.0) for c in cams]
    fps[3] = (fps[3][0], fps[3][1], fps[3][2] + 400, fps[3][3])            # frame 3 sees much farther
    s = WD.snap_out(fps[0], 32)
    with pytest.raises(ValueError, match=r"frame 3 .*%d pixels" % (WD.snap_out(fps[3], 32)[2] * WD.snap_out(fps[3], 32)[3])):
        WD.plan_windows(fps, 32, 2 * s[2] * s[3])
    with pytest.raises(ValueError, match="frame 0"):
        WD.plan_windows(fps, 32, s[2] * s[3] - 1)
    for bad in (0, -32, 2.0, True):
        with pytest.raises(ValueError, match="snap"):
            WD.plan_windows(fps, bad, 10 ** 9)


def test_flight_plan_derives_the_cap_and_the_snap_from_the_world():
    w = _world(chunk_cells=2)                                              # in_shp = 32; no engine, no device
    cams = _line(12, (-200.0, 11.25, 14.0), (200.0, 11.25, 14.0))
    fps = [c.footprint(40.0) for c in cams]
    assert WD.SCENE_BYTES_PER_PIXEL == 22 and 4 + 12 + 16 / 3.0 <= WD.SCENE_BYTES_PER_PIXEL < 4 + 12 + 16 / 3.0 + 1
    mb = 128 * 128 * 22 / float(1 << 20)
    cap = int(mb * (1 << 20)) // 22
    assert cap == 128 * 128
    plan = w.flight_plan(cams, 40.0, window_mb=mb)
    assert plan == WD.plan_windows(fps, 32, cap) and len(plan) >= 3
    _check_plan(plan, fps, 32, cap)
    assert w.flight_plan(cams, 40.0, window_mb=mb, snap=16) == WD.plan_windows(fps, 16, cap)
    assert len(w.flight_plan(cams, 40.0)) == 1                             # the default gigabyte holds this path
    assert w.flight_plan(iter(cams), 40.0, window_mb=mb) == plan
    for bad in (0, -1.0, None, True, float('nan')):
        with pytest.raises(ValueError, match="window_mb"):
            w.flight_plan(cams, 40.0, window_mb=bad)
    with pytest.raises(ValueError, match="frame 0"):
        w.flight_plan(cams, 40.0, window_mb=0.001)
    # flight itself plans, and refuses, before it touches a device: this world has none
    with pytest.raises(ValueError, match="frame 0"):
        w.flight(cams, 40.0, window_mb=0.001)
    assert w.computed == 0
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.flight(cams, 40.0)
    with pytest.raises(ValueError, match="closed"):
        w.scene(0, 0, 64, 64, resident=True)


WORLD_ARGS = ["o.png", "--world", "test1_nobn_bilin_both", "m.model", "--seed", "7", "--pos", "-10,64,50", "--yaw", "0",
              "--pitch", "-30", "--max-dist", "200"]


def test_cli_window_mb_arguments():
    a = RN.parse_args(WORLD_ARGS + ["--frames", "3", "--to", "400,64,50", "--window-mb", "64"])
    assert a.window_mb == 64.0 and a.frames == 3
    assert RN.parse_args(WORLD_ARGS + ["--frames", "3", "--to", "400,64,50"]).window_mb is None
    assert RN.parse_args(WORLD_ARGS).window_mb is None
    for bad in (WORLD_ARGS + ["--window-mb", "64"],                                            # no path
                WORLD_ARGS + ["--frames", "3", "--to", "400,64,50", "--window-mb", "0"],
                WORLD_ARGS + ["--frames", "3", "--to", "400,64,50", "--window-mb", "-1"],
                ["o.png", "--heightmap", "h.png", "--texture", "t.png", "--pos", "0,0,9", "--yaw", "0", "--pitch", "-30",
                 "--frames", "3", "--to", "40,6,9", "--window-mb", "64"]):                       # no world
        with pytest.raises(SystemExit):
            RN.parse_args(bad)


def test_cli_dispatches_a_windowed_path_to_flight(tmp_path, monkeypatch):
    """main() with --window-mb renders through TerrainWorld.flight with the path's cameras and the window size, and writes
    the frames it yields; without it, through one union scene as before"""
    from gan_heightmaps_amd import experiments, util
    calls, saved = [], []

    class Dev:
        def close(self):
            pass

    class Scene:
        def render(self, cam, **kw):
            return ("scene", cam.pos)

        def close(self):
            pass

    class World:
        def flight(self, cams, max_dist, **kw):
            calls.append(("flight", len(cams), max_dist, kw))
            return iter([("flight", c.pos) for c in cams])

        def scene(self, *rect, **kw):
            calls.append(("scene", rect, kw))
            return Scene()

        def close(self):
            pass

    class Model:
        device = Dev()

        def load_model(self, path, mode):
            pass

        def terrain_world(self, seed, **kw):
            return World()

    monkeypatch.setattr(experiments, "make_model", lambda name, **kw: Model())
    monkeypatch.setattr(util, "save_png", lambda name, img: saved.append((name, img)))
    out = str(tmp_path / "o.png")
    args = [out] + WORLD_ARGS[1:] + ["--frames", "3", "--to", "400,64,50", "--height-scale", "10", "--no-shadows"]
    assert RN.main(args + ["--window-mb", "2.5"]) == 0
    assert [c[0] for c in calls] == ["flight"]
    _, n, max_dist, kw = calls[0]
    assert (n, max_dist, kw["window_mb"], kw["height_scale"], kw["shadows"]) == (3, 200.0, 2.5, 10.0, False)
    assert "max_dist" not in kw
    assert [s[0] for s in saved] == [out[:-4] + "_%04d.png" % i for i in range(3)]
    assert [s[1][0] for s in saved] == ["flight"] * 3 and saved[2][1][1] == (400.0, 64.0, 50.0)
    del calls[:], saved[:]
    assert RN.main(args) == 0
    assert [c[0] for c in calls] == ["scene"] and [s[1][0] for s in saved] == ["scene"] * 3
    cams = RN.cameras_of(RN.parse_args(args))
    assert calls[0][1] == RN.union_footprint([c.footprint(200.0) for c in cams])
    assert math.isclose(np.float64(calls[0][2]["height_scale"]), 10.0)
