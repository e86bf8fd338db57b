"""The host side of the earthworks (gan_heightmaps_amd/earthworks.py): Profile's, Channel's and Roadbed's validation,
the table and the target builders against the restatement, the refusals that are made before the device is touched, the command
lines' parsing.  And the device code of csrc/earthworks.hip compiled for the CPU (tests/earthworks_host/harness.cpp): the same
source text the GPU runs, the tiled form phase by phase, both forms and the shaping bit for bit against tests/earthworks_ref.py on
the planes of the device tests, once more under the address and undefined-behaviour sanitizers.  No device."""
import os
import subprocess

import numpy as np
import pytest

from gan_heightmaps_amd import earthworks as EW
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import route as RT
from tests import earthworks_ref as E
from tests import hydrology_ref as HR
from tests import route_ref as RR
from tests.test_render_host import CSRC, ROOT, _compiler


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_profile_validation_and_table():
    p = EW.Profile(1, np.float32(6.5), 'cut')
    assert (p.core, p.reach, p.mode, p.R, p.mode_index) == (1.0, 6.5, 'cut', 6, 1) and hash(p) == hash(EW.Profile(1.0, 6.5, 'cut'))
    assert EW.Profile(0, 0).R == 0 and EW.Profile(32, 32).R == 32 and EW.Profile(0.5, 0.75).R == 0
    with pytest.raises(Exception):
        p.core = 2                                                        # frozen
    for args in ((-0.1, 2), (3, 2), (1, 32.5), (1, float("inf")), (float("nan"), 2), (1, None), (True, 2), ("1", 2), (1, 2, 'dig'),
                 (1, 2, 0)):
        with pytest.raises(ValueError):
            EW.Profile(*args)
    for core, reach in ((0.0, 4.0), (1.0, 6.0), (2.0, 2.0), (0.0, 0.0), (1.5, 2.5), (0.25, 32.0), (32.0, 32.0), (3.0, 7.9)):
        t = EW.Profile(core, reach).table()
        assert t.dtype == np.float32 and t.flags.c_contiguous and t.tobytes() == E.table(core, reach).tobytes(), (core, reach)
    assert EW.MODES == E.MODES and EW.MAX_REACH == E.MAX_REACH and EW.NONE == E.NONE and EW.TILE == E.TILE


def test_channel_and_roadbed_validation():
    c = EW.Channel()
    assert (c.river_threshold, c.lake_min_depth, c.depth, c.growth, c.max_depth, c.core, c.reach, c.height_scale) == \
        (256, 1.0 / 512, 0.5, 0.25, 3.0, 0.0, 4.0, 64.0)
    assert c.profile == EW.Profile(0.0, 4.0, 'cut')
    assert EW.Channel(river_threshold=np.int32(9), depth=1, reach=np.float64(3)) == EW.Channel(river_threshold=9, depth=1.0, reach=3.0)
    for kw in (dict(river_threshold=0), dict(river_threshold=1 << 32), dict(river_threshold=2.0), dict(river_threshold=True),
               dict(lake_min_depth=-1), dict(depth=-0.1), dict(depth=float("nan")), dict(growth=float("inf")), dict(max_depth=-1),
               dict(core=5.0), dict(reach=33), dict(core=-1), dict(height_scale=0), dict(height_scale=float("inf")),
               dict(height_scale=1e-39), dict(depth=None)):
        with pytest.raises(ValueError):
            EW.Channel(**kw)
    r = EW.Roadbed()
    assert (r.core, r.reach, r.smooth, r.mode) == (1.0, 6.0, 8, 'both') and r.profile == EW.Profile(1.0, 6.0, 'both')
    assert EW.Roadbed(smooth=np.int64(0), mode='fill').profile.mode_index == 2
    with pytest.raises(Exception):
        r.smooth = 2
    for kw in (dict(core=7.0), dict(reach=40), dict(smooth=-1), dict(smooth=2.0), dict(smooth=True), dict(smooth=EW.MAX_SMOOTH + 1),
               dict(mode='level'), dict(core=float("nan"))):
        with pytest.raises(ValueError):
            EW.Roadbed(**kw)


# ---- the target builders against the restatement -----------------------------------------------------------------------------------
def test_channel_targets_equal_the_restatement():
    H, W, q, seed = HR.CASES[1]
    r = HR.analyse(HR.terrain(H, W, q, seed))
    ch = EW.Channel(river_threshold=40, lake_min_depth=1.0 / 64, depth=0.4, growth=0.3, max_depth=1.1, height_scale=48)
    marks, target = EW.channel_targets(r.filled, r.depth, r.accumulation, ch)
    wm, wt = E.channel_targets(r.filled, r.depth, r.accumulation, 40, 1.0 / 64, 0.4, 0.3, 1.1, 48.0)
    assert marks.dtype == np.uint32 and target.dtype == np.float32
    assert np.array_equal(marks, wm) and target.tobytes() == wt.tobytes() and 20 < int(marks.sum()) < H * W // 4
    big = np.array([[1, 3, 4, 1 << 31, 0xFFFFFFFF]], np.uint32)
    z = np.zeros((1, 5), np.float32)
    got = EW.channel_targets(z, z, big, EW.Channel(river_threshold=1, max_depth=30.0))[1]
    assert got.tobytes() == E.channel_targets(z, z, big, 1, max_depth=30.0)[1].tobytes() and got[0, 4] == np.float32(-8.25 / 64)


def test_road_targets_equal_the_restatement():
    h, pen, sources = RR.case(3, 5)
    r = RR.field(h, sources, penalty=pen)
    cells = [tuple(int(v) for v in c) for c in np.argwhere(r.cost != RR.UNREACHED)[::173]]
    seeds = RR.raster(h.shape, [RR.walk(r.parent, c) for c in cells]) != 0
    ends = np.zeros(h.shape, bool)
    for c in cells:
        ends[c] = True
    ends[tuple(np.argwhere(r.cost == RR.UNREACHED)[0])] = True                    # an unreached cell: a road of one cell
    for smooth in (0, 1, 8, 200):
        for s in (seeds, ends, r.traffic >= 25):
            marks, target = EW.road_targets(h, r.parent, s, EW.Roadbed(smooth=smooth))
            wm, wt = E.road_targets(h, r.parent, s, smooth)
            assert np.array_equal(marks, wm) and target.tobytes() == wt.tobytes(), smooth
    assert int(marks.sum()) > 40


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    h = E.heights(8, 9, 1)
    marks = np.zeros((8, 9), np.uint32)
    marks[2, 3] = 1
    target = np.full((8, 9), np.nan, np.float32)
    target[2, 3] = 0.5
    prof = EW.Profile(1, 3)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            EW.carve(ops, bad, marks, target, prof)
    for v in (np.nan, np.inf, -np.inf):
        x = h.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match="non-finite"):
            EW.carve(ops, x, marks, target, prof)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    tall = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(4 * 65535 + 1, 2), strides=(0, 0), writeable=False)
    for x in (huge, tall):
        with pytest.raises(ValueError, match="out of range"):
            EW.carve(ops, x, marks, target, prof)
        with pytest.raises(ValueError, match="out of range"):
            EW.nearest(ops, np.lib.stride_tricks.as_strided(np.zeros(1, np.uint32), shape=x.shape, strides=(0, 0)), 2)
    for bad in (np.zeros((9, 8), np.uint32), np.zeros((8, 9), np.float32), np.zeros(72, np.uint32), np.full((8, 9), -1, np.int32)):
        with pytest.raises(ValueError, match="marks"):
            EW.carve(ops, h, bad, target, prof)
    for bad in (np.zeros((9, 8), np.float32), np.zeros((8, 9), np.int32)):
        with pytest.raises(ValueError, match="target"):
            EW.carve(ops, h, marks, bad, prof)
    for v in (np.nan, np.inf):                                            # non-finite at a marked cell; elsewhere it may be
        t = target.copy()
        t[2, 3] = v
        with pytest.raises(ValueError, match="marked"):
            EW.carve(ops, h, marks, t, prof)
    with pytest.raises(ValueError, match="marked"):
        EW.carve(ops, h, marks + np.uint32(2), target, prof, threshold=2)  # every cell is marked now, and most targets are NaN
    for bad in (0, -1, 1 << 32, 1.0, True):
        with pytest.raises(ValueError, match="threshold"):
            EW.carve(ops, h, marks, target, prof, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            EW.nearest(ops, marks, 2, threshold=bad)
    for bad in (-1, 33, 2.0, None, True):
        with pytest.raises(ValueError, match="reach"):
            EW.nearest(ops, marks, bad)
    for bad in (None, dict(core=1, reach=2), EW.Roadbed()):
        with pytest.raises(ValueError, match="Profile"):
            EW.carve(ops, h, marks, target, bad)
    with pytest.raises(ValueError, match="keep"):
        EW.carve(ops, h, marks, target, prof, keep=('height', 'marks'))
    # cut_rivers and grade_roads
    z = np.zeros((8, 9), np.float32)
    for bad in (None, h, HY.Hydrology((8, 9), (1, 1), 1, False, filled=h, depth=z),
                HY.Hydrology((8, 9), (1, 1), 1, False, depth=z, accumulation=marks)):
        with pytest.raises(ValueError, match="filled"):
            EW.cut_rivers(ops, bad)
    hydro = HY.Hydrology((8, 9), (1, 1), 1, False, filled=h, depth=z, accumulation=marks)
    with pytest.raises(ValueError, match="Channel"):
        EW.cut_rivers(ops, hydro, channel=dict(depth=1))
    parent = np.full((8, 9), -1, np.int8)
    cf = RT.CostField((8, 9), [(0, 0)], parent=parent)
    for bad in (None, RT.CostField((8, 9), [(0, 0)], cost=marks)):
        with pytest.raises(ValueError, match="parent"):
            EW.grade_roads(ops, h, bad)
    with pytest.raises(ValueError, match="differ in size"):
        EW.grade_roads(ops, h.T.copy(), cf)
    with pytest.raises(ValueError, match="Roadbed"):
        EW.grade_roads(ops, h, cf, roadbed=EW.Channel())
    with pytest.raises(ValueError, match="traffic"):
        EW.grade_roads(ops, h, cf, traffic_threshold=3)
    for bad in (0, 1 << 32, 2.5):
        with pytest.raises(ValueError, match="traffic_threshold"):
            EW.grade_roads(ops, h, RT.CostField((8, 9), [(0, 0)], parent=parent, traffic=marks), traffic_threshold=bad)
    with pytest.raises(ValueError, match="leaves the plane"):
        EW.grade_roads(ops, h, cf, [np.array([[0, 0], [8, 0]])])
    with pytest.raises(ValueError, match="leaves the plane"):
        EW.grade_roads(ops, h, RT.CostField((8, 9), [(5, 5)], origin=(5, 5), parent=parent), [np.array([[0, 0]])])


def test_carve_sends_two_launches_inside_one_scratch():
    from tests.fake_device import FakeDevice, RecordingOps
    ops = RecordingOps(FakeDevice())
    h = E.heights(8, 9, 1)
    marks = np.zeros((8, 9), np.uint32)
    marks[2, 3] = 5
    e = EW.carve(ops, h[None], marks, np.zeros((8, 9), np.float64), EW.Profile(1, 3.5, 'fill'), threshold=4, tiled=False,
                 keep=('height', 'dist2'), origin=(3, -4))
    assert [c[0] for c in ops.calls] == ["earthworks_nearest", "earthworks_shape"]
    near, shape = ops.calls[0][1], ops.calls[1][1]
    assert near[1:7] == (9, 8, 9, 4, 3, False) and near[8] == near[10] == 9
    assert shape[9:13] == (3, 2, 8, 9) and shape[2] == near[7] and shape[4] == near[9] and shape[14] == 9
    assert ops.dev.uploads == 4 and e.shape == (8, 9) and e.origin == (3, -4) and e.tiled is False
    assert e.nearest is None and e.height.shape == e.dist2.shape == (8, 9) and "Earthworks" in repr(e)
    ops = RecordingOps(FakeDevice())
    n, d = EW.nearest(ops, marks, 7, threshold=5)
    assert [c[0] for c in ops.calls] == ["earthworks_nearest"] and ops.calls[0][1][4:7] == (5, 7, EW.DEFAULT_TILED)
    assert n.dtype == d.dtype == np.int32 and n.shape == (8, 9)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = EW.parse_args(["in.png", "out.npy", "--rivers"])
    assert (a.input, a.output, a.rivers, a.sources, a.targets, a.traffic_threshold, a.form) == \
        ("in.png", "out.npy", True, [], [], None, None)
    assert a.channel == EW.Channel() and a.roadbed == EW.Roadbed() and a.travel == RT.Travel()
    a = EW.parse_args(["i.npy", "o.png", "--rivers", "--from", "1,2", "--from", "30,40", "--to", "5,6", "--channel-depth", "1",
                       "--channel-growth", "0.5", "--channel-max-depth", "2", "--river-threshold", "64", "--lake-min-depth", "0.01",
                       "--river-core", "1", "--river-reach", "3", "--road-core", "0", "--road-reach", "2.5", "--road-smooth", "4",
                       "--road-mode", "cut", "--height-scale", "32", "--tiled"])
    assert a.sources == [(1, 2), (30, 40)] and a.targets == [(5, 6)] and a.form is True
    assert a.channel == EW.Channel(river_threshold=64, lake_min_depth=0.01, depth=1, growth=0.5, max_depth=2, core=1, reach=3,
                                   height_scale=32)
    assert a.roadbed == EW.Roadbed(core=0, reach=2.5, smooth=4, mode='cut')
    assert a.travel == RT.Travel(river_threshold=64, lake_min_depth=0.01, height_scale=32)
    a = EW.parse_args(["i", "o", "--from", "0,0", "--traffic-threshold", "50", "--plain"])
    assert a.form is False and a.traffic_threshold == 50 and not a.rivers
    for bad in (["i", "o"], ["i", "--rivers"], ["i", "o", "--to", "1,2"], ["i", "o", "--rivers", "--to", "1,2"],
                ["i", "o", "--from", "1,2"], ["i", "o", "--rivers", "--traffic-threshold", "5"],
                ["i", "o", "--from", "1,2", "--traffic-threshold", "0"], ["i", "o", "--rivers", "--plain", "--tiled"],
                ["i", "o", "--rivers", "--river-reach", "33"], ["i", "o", "--rivers", "--river-core", "5"],
                ["i", "o", "--rivers", "--road-mode", "level"], ["i", "o", "--rivers", "--road-smooth", "-1"],
                ["i", "o", "--rivers", "--height-scale", "0"], ["i", "o", "--from", "1", "--to", "1,2"]):
        with pytest.raises(SystemExit):
            EW.parse_args(bad)


def test_the_worlds_command_line_takes_earthworks():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    assert WD.parse_args(base).earthworks is None
    assert WD.parse_args(base + ["--earthworks", "ground.npy"]).earthworks == "ground.npy"
    a = WD.parse_args(base + ["--earthworks", "g.png", "--routes", "pre", "--from", "-5,40", "--to", "-60,35"])
    assert a.earthworks == "g.png" and a.sources == [(-5, 40)] and a.targets == [(-60, 35)]
    assert WD.WorldEarthworks(1, 2, 3, 4).paths == 4


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "earthworks.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "earthworks.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           '-DEARTHWORKS_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "earthworks_host", "harness.cpp"),
                                                                 "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("earthworks_host")
    exe, r = _build(d, "earthworks_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run(harness, marks, threshold, R, h=None, target=None, table=None, mode=0):
    """-> (nearest, dist2 of the plain form, of the tiled form, the shaped heights); inputs in rows of W + 3 cells with marked and
    NaN padding, outputs in rows of W + 2 cells whose padding must come back untouched"""
    d, exe = harness
    H, W = marks.shape
    pi, po = W + 3, W + 2
    h = np.zeros((H, W), np.float32) if h is None else h
    target = np.zeros((H, W), np.float32) if target is None else target
    table = E.table(0.0, float(R)) if table is None else table
    assert table.shape == (R * R + 1, 2)
    planes = []
    for plane, dtype, fill in ((marks, np.uint32, 0xFFFFFFFF), (h, np.float32, np.nan), (target, np.float32, np.nan)):
        wide = np.full((H, pi), fill, dtype)
        wide[:, :W] = plane
        planes.append(wide.tobytes())
    (d / "in.bin").write_bytes(b"".join(planes) + np.ascontiguousarray(table, np.float32).tobytes())
    args = ["run", H, W, pi, po, R, threshold, mode, d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.frombuffer((d / "out.bin").read_bytes(), np.uint8).reshape(5, H, po * 4)
    assert (raw[:, :, W * 4:] == 0xAB).all(), "cells beyond a row's width were written"
    body = np.ascontiguousarray(raw[:, :, :W * 4])
    ints = body[:4].view(np.int32).reshape(4, H, W)
    return ints[0], ints[1], ints[2], ints[3], body[4].view(np.float32).reshape(H, W)


@pytest.mark.parametrize("kind", E.KINDS)
def test_both_forms_of_the_nearest_mark_on_the_host_build(harness, kind):
    for shape, R in E.nearest_cases():
        m, thr, near, dist2 = E.nearest_case(kind, shape, R)
        pn, pd, tn, td, _ = run(harness, m, thr, R)
        assert np.array_equal(pn, near) and np.array_equal(pd, dist2), (kind, shape, R, "plain")
        assert np.array_equal(tn, near) and np.array_equal(td, dist2), (kind, shape, R, "tiled")


@pytest.mark.parametrize("mode", range(3))
def test_the_shaping_on_the_host_build(harness, mode):
    for shape, (core, reach) in (((1, 1), (0.0, 0.0)), ((1, 40), (1.0, 5.5)), ((31, 33), (2.0, 2.0)), ((33, 65), (0.0, 32.0)),
                                 ((70, 45), (1.0, 6.0)), ((64, 64), (0.0, 0.0))):
        R = int(reach)
        h, m, thr, target = E.shape_case(shape, R, 7 + mode)
        tab = E.table(core, reach)
        near, dist2 = E.nearest(m, R, thr)
        want = E.shape(h, near, dist2, target, tab, mode)
        got = run(harness, m, thr, R, h, target, tab, mode)
        assert np.array_equal(got[2], near) and got[4].tobytes() == want.tobytes(), (shape, core, reach)
        assert np.isnan(target).any() or shape == (1, 1)
        assert np.isfinite(got[4]).all()


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: out-of-bounds LDS or plane indices and signed overflow
    in the kernels' index arithmetic end it"""
    exe, r = _build(tmp_path, "earthworks_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    for kind in ('corners', 'checker', 'scatter'):
        for shape, R in (((1, 1), 0), ((1, 40), 5), ((40, 1), 5), ((31, 33), 1), ((33, 65), 32), ((70, 45), 5)):
            m, thr, near, dist2 = E.nearest_case(kind, shape, R)
            h, _, _, _ = E.shape_case(shape, R, 3)
            target = np.where(m.astype(np.int64) >= thr, np.float32(0.25), np.float32(np.nan)).astype(np.float32)
            tab = E.table(0.0, float(R))
            got = run((tmp_path, exe), m, thr, R, h, target, tab, 0)
            assert np.array_equal(got[0], near) and np.array_equal(got[3], dist2)
            assert got[4].tobytes() == E.shape(h, near, dist2, target, tab, 0).tobytes()
