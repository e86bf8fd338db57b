"""The host side of the route module (gan_heightmaps_amd/route.py): Travel's and Road's validation, the refusals
that are made before the device is touched, path and paths on a hand-made CostField, the rasteriser, and the command lines'
parsing.  No device."""
import math

import numpy as np
import pytest

from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import route as RT
from tests import route_ref as R


def test_travel_defaults_and_validation():
    t = RT.Travel()
    assert (t.grade, t.lake, t.ford, t.river_threshold, t.lake_min_depth, t.height_scale) == (0.15, 16.0, 4.0, 256, 1.0 / 512, 64.0)
    assert RT.Travel(grade=np.float32(0.5), lake=np.int64(2), ford=1, river_threshold=np.int32(7), height_scale=8) == \
        RT.Travel(grade=0.5, lake=2.0, ford=1.0, river_threshold=7, height_scale=8.0)
    assert RT.Travel(lake=float("inf")).lake == math.inf and hash(RT.Travel()) == hash(RT.Travel())
    with pytest.raises(Exception):
        t.grade = 0.5                                                     # frozen
    for kw in (dict(grade=0), dict(grade=-0.1), dict(grade=float("inf")), dict(grade=float("nan")), dict(grade=None),
               dict(grade=True), dict(grade=1e-39), dict(height_scale=0), dict(height_scale=-1), dict(height_scale=float("inf")),
               dict(height_scale=float("nan")), dict(lake=0.5), dict(lake=float("nan")), dict(lake=-float("inf")),
               dict(lake="16"), dict(ford=0.9), dict(ford=float("inf")), dict(ford=float("nan")), dict(river_threshold=0),
               dict(river_threshold=1 << 32), dict(river_threshold=2.0), dict(river_threshold=True), dict(lake_min_depth=-1e-3),
               dict(lake_min_depth=float("nan")), dict(lake_min_depth=float("inf"))):
        with pytest.raises(ValueError):
            RT.Travel(**kw)


def test_road_defaults_and_validation():
    r = RT.Road()
    assert (r.width, r.colour, r.opacity, r.traffic_threshold) == (1, (0.35, 0.30, 0.25), 0.9, None)
    assert RT.Road(width=np.int32(HY.MAX_RIVER_WIDTH), colour=[0, 1, 0.5], opacity=1, traffic_threshold=np.int64(9)) == \
        RT.Road(width=4, colour=(0.0, 1.0, 0.5), opacity=1.0, traffic_threshold=9)
    with pytest.raises(Exception):
        r.width = 2
    for kw in (dict(width=-1), dict(width=HY.MAX_RIVER_WIDTH + 1), dict(width=1.0), dict(opacity=1.5), dict(opacity=-0.1),
               dict(opacity=None), dict(colour=(0.1, 0.2)), dict(colour=(0.1, 0.2, 1.5)), dict(colour=0.3),
               dict(colour=(0.1, 0.2, float("nan"))), dict(traffic_threshold=0), dict(traffic_threshold=1 << 32),
               dict(traffic_threshold=2.5), dict(traffic_threshold=True)):
        with pytest.raises(ValueError):
            RT.Road(**kw)


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    good = R.terrain(8, 9, None, 1)
    src = [(1, 2)]
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            RT.field(ops, bad, src)
    for v in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match="non-finite"):
            RT.field(ops, x, src)
    # H W >= 2^31 by shape arithmetic alone: a view of one float, never read
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        RT.field(ops, huge, src)
    tall = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(4 * 65535 + 1, 2), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        RT.field(ops, tall, src)
    for bad in ([], [(8, 0)], [(0, 9)], [(-1, 0)], [(1.5, 2)], [(1, 2, 3)], 5, [(1, 2)] * (RT.MAX_SOURCES + 1), [(True, 1)]):
        with pytest.raises(ValueError, match="source"):
            RT.field(ops, good, bad)
    with pytest.raises(ValueError, match="source"):
        RT.field(ops, good, [(1, 2)], origin=(5, 5))                      # sources come in the origin's coordinates
    with pytest.raises(ValueError, match="keep"):
        RT.field(ops, good, src, keep=("cost", "roads"))
    with pytest.raises(ValueError, match="Travel"):
        RT.field(ops, good, src, travel=dict(grade=1))
    for bad in (np.ones((9, 8), np.float32), np.ones((8, 9), np.int32), np.full((8, 9), 0.5, np.float32),
                np.full((8, 9), np.nan, np.float32), np.full((8, 9), -np.inf, np.float32)):
        with pytest.raises(ValueError, match="penalty"):
            RT.field(ops, good, src, penalty=bad)
    with pytest.raises(ValueError, match="depth"):
        RT.field(ops, good, src, hydro=HY.Hydrology((8, 9), (1, 1), 1, False, filled=good))
    with pytest.raises(ValueError, match="depth"):
        RT.field(ops, good, src, hydro=good)
    hydro = HY.Hydrology((9, 8), (1, 1), 1, False, depth=np.zeros((9, 8), np.float32), accumulation=np.ones((9, 8), np.uint32))
    with pytest.raises(ValueError, match="differ in size"):
        RT.field(ops, good, src, hydro=hydro)
    # paint: the road and the field are checked first, then the paths, then the texture's form and size
    cf = RT.CostField((8, 9), src, traffic=np.ones((8, 9), np.uint32))
    tex = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError, match="Road"):
        RT.paint(ops, tex, cf, road=dict(width=1))
    with pytest.raises(ValueError, match="CostField"):
        RT.paint(ops, tex, None)
    with pytest.raises(ValueError, match="traffic"):
        RT.paint(ops, tex, RT.CostField((8, 9), src), road=RT.Road(traffic_threshold=3))
    with pytest.raises(ValueError, match="leaves the plane"):
        RT.paint(ops, tex, cf, [np.array([[0, 0], [8, 0]])])
    with pytest.raises(ValueError, match="path"):
        RT.paint(ops, tex, cf, [np.zeros((3, 2), np.float32)])
    with pytest.raises(ValueError, match="differ in size"):
        RT.paint(ops, np.zeros((9, 8, 3), np.uint8), cf)
    for bad in (np.zeros((8, 9, 2), np.uint8), np.zeros((2, 8, 9), np.float32), np.zeros((8, 9), np.float64),
                np.full((8, 9), np.nan, np.float32)):
        with pytest.raises(ValueError):
            RT.paint(ops, bad, cf)


def test_both_paints_make_one_launch_with_the_arguments_they_always_sent():
    """hydrology.paint and route.paint on a device of fake addresses (they encode the order and the sizes of the four
    allocations) and recording ops: one hydrology_paint call each, its arguments the literals recorded from the two paints
    as they were before they shared one"""
    from tests.fake_device import FakeDevice, RecordingOps
    hydro = HY.Hydrology((8, 9), (1, 1), 1, False, depth=np.zeros((8, 9), np.float32), accumulation=np.ones((8, 9), np.uint32))
    cf = RT.CostField((8, 9), [(1, 2)], traffic=np.ones((8, 9), np.uint32))
    path = np.array([[0, 0], [1, 1], [2, 1]], np.int32)
    water, road = (0.12999999523162842, 0.28999999165534973, 0.44999998807907104), (0.3499999940395355, 0.30000001192092896, 0.25)
    for tex, C, u8, out_ptr in ((np.zeros((8, 9, 3), np.uint8), 3, True, 1051392), (np.zeros((8, 9), np.float32), 1, False, 1050880)):
        head = (1048576, 9, 1049344, 9, 8, 9, 1050112, 9, C)
        for paint, args, want in (
                (HY.paint, (hydro, HY.Water(river_threshold=5, river_width=2, lake_min_depth=0.25, opacity=0.5)),
                 head + (water, 0.5, 0.25, 5, 2, u8, out_ptr, 9)),
                (RT.paint, (cf, [path], RT.Road(width=3)), head + (road, 0.9, 0.0, 1, 3, u8, out_ptr, 9)),
                (RT.paint, (cf, (), RT.Road(width=0, opacity=0.25, traffic_threshold=7)),
                 head + (road, 0.25, 0.0, 7, 0, u8, out_ptr, 9))):
            ops = RecordingOps(FakeDevice())
            out = paint(ops, tex, *args)
            assert ops.calls == [("hydrology_paint", want, {})], (paint.__module__, tex.dtype)
            assert ops.dev.uploads == 3 and (out.dtype, out.shape) == (tex.dtype, tex.shape)
            assert all(type(v) is type(w) for v, w in zip(ops.calls[0][1], want))      # 1 is not True, 0.0 is not 0


def hand_field(origin=(0, 0)):
    """a 3 x 4 field by hand: the source at (1, 1), the last column unreached"""
    parent = np.array([[3, 4, 5, -2], [2, -1, 6, -2], [1, 0, 7, -2]], np.int8)
    cost = np.array([[91, 64, 91, R.UNREACHED], [64, 0, 64, R.UNREACHED], [91, 64, 91, R.UNREACHED]], np.uint32)
    return RT.CostField((3, 4), [(1 + origin[0], 1 + origin[1])], origin, 5, True, cost=cost, parent=parent)


def test_path_and_paths_on_a_hand_made_field():
    f = hand_field()
    assert f.unit == 64 and f.shape == (3, 4) and f.origin == (0, 0) and f.sweeps == 5 and f.tiled is True
    assert f.territory is None and f.traffic is None and "CostField" in repr(f)
    p = f.path((0, 0))
    assert p.dtype == np.int32 and p.tolist() == [[0, 0], [1, 1]]
    assert f.path((1, 1)).tolist() == [[1, 1]] and f.path((2, 2)).tolist() == [[2, 2], [1, 1]]
    assert [q.tolist() for q in f.paths([(0, 1), (1, 2)])] == [[[0, 1], [1, 1]], [[1, 2], [1, 1]]] and f.paths([]) == []
    assert f.travel_cost((0, 0)) == 91 / 64.0 and f.travel_cost((1, 1)) == 0.0 and f.travel_cost((0, 3)) == math.inf
    with pytest.raises(ValueError, match="unreached"):
        f.path((1, 3))
    for bad in ((3, 0), (0, 4), (-1, 0), (0.5, 1), 7):
        with pytest.raises(ValueError):
            f.path(bad)
    with pytest.raises(ValueError, match="parent"):
        RT.CostField((3, 4), [(1, 1)], cost=f.cost).path((0, 0))
    with pytest.raises(ValueError, match="cost"):
        RT.CostField((3, 4), [(1, 1)], parent=f.parent).travel_cost((0, 0))
    # with an origin, cells go in and come out in its coordinates
    g = hand_field((-10, 100))
    assert g.path((-10, 100)).tolist() == [[-10, 100], [-9, 101]] and g.travel_cost((-9, 101)) == 0.0
    with pytest.raises(ValueError, match="outside"):
        g.path((0, 0))
    # a longer walk equals the restatement's
    h, pen, src = R.case(3, 5)
    r = R.field(h, src, penalty=pen)
    f = RT.CostField(h.shape, src, cost=r.cost, parent=r.parent)
    for cell in [tuple(c) for c in np.argwhere(r.cost != R.UNREACHED)[::97]]:
        assert np.array_equal(f.path(cell), R.walk(r.parent, cell))
        assert f.travel_cost(cell) == int(r.cost[cell]) / 64.0
    # a parent plane that is no forest is refused, not walked for ever
    loop = RT.CostField((1, 2), [(0, 0)], parent=np.array([[2, 6]], np.int8))
    with pytest.raises(ValueError, match="forest"):
        loop.path((0, 0))


def test_the_rasteriser_and_the_territory_map():
    paths = [np.array([[0, 0], [1, 1], [2, 1]], np.int32), np.zeros((0, 2), np.int32), np.array([[2, 3]])]
    m = RT.raster((3, 4), paths)
    assert m.dtype == np.uint32 and np.array_equal(m, R.raster((3, 4), paths)) and int(m.sum()) == 4
    assert np.array_equal(RT.raster((3, 4), [p + np.array([5, -7]) for p in paths], origin=(5, -7)), m)
    assert RT.raster((3, 4), ()).sum() == 0
    for bad in ([np.array([[3, 0]])], [np.array([[0, -1]])], [np.array([0, 1])], [np.array([[0.0, 1.0]])]):
        with pytest.raises(ValueError):
            RT.raster((3, 4), bad)
    # the map from the accumulation's roots to the sources' ordinals; duplicates keep the lowest
    h, pen, src = R.case(3, 5)
    src = [src[0]] + src
    r = R.field(h, src, penalty=pen)
    H, W = h.shape
    from tests import hydrology_ref as HR
    acc, basin, _ = HR.doubling(np.where(r.parent >= 0, r.parent, -1).astype(np.int8))
    terr, traffic = RT.territory_traffic(basin, acc, r.cost, R.flat_sources(src, W))
    assert terr.dtype == np.int32 and traffic.dtype == np.uint32
    assert np.array_equal(terr, r.territory) and np.array_equal(traffic, r.traffic) and 1 not in terr


def test_command_line_parsing():
    a = RT.parse_args(["in.png", "out/prefix", "--from", "3,4"])
    assert (a.input, a.out_prefix, a.sources, a.targets, a.hydrology, a.texture, a.painted, a.form) == \
        ("in.png", "out/prefix", [(3, 4)], [], False, None, None, None)
    assert a.travel == RT.Travel() and a.road == RT.Road()
    a = RT.parse_args(["in.npy", "p", "--from", "1,2", "--from", " 30 , 40 ", "--to", "5,6", "--to", "7,8", "--hydrology", "--texture",
                       "t.png", "--painted", "o.png", "--road-width", "2", "--traffic-threshold", "50", "--grade", "0.3", "--lake",
                       "inf", "--ford", "2", "--river-threshold", "64", "--lake-min-depth", "0.01", "--height-scale", "32",
                       "--tiled"])
    assert a.sources == [(1, 2), (30, 40)] and a.targets == [(5, 6), (7, 8)] and a.hydrology and a.form is True
    assert a.travel == RT.Travel(grade=0.3, lake=math.inf, ford=2, river_threshold=64, lake_min_depth=0.01, height_scale=32)
    assert a.road == RT.Road(width=2, traffic_threshold=50) and (a.texture, a.painted) == ("t.png", "o.png")
    assert RT.parse_args(["i", "p", "--from", "0,0", "--plain"]).form is False
    for bad in (["i", "p"], ["i", "--from", "1,2"], ["i", "p", "--from", "1"], ["i", "p", "--from", "1,2,3"],
                ["i", "p", "--from", "1,2", "--plain", "--tiled"], ["i", "p", "--from", "1,2", "--texture", "t.png"],
                ["i", "p", "--from", "1,2", "--painted", "o.png"], ["i", "p", "--from", "1,2", "--road-width", "2"],
                ["i", "p", "--from", "1,2", "--grade", "0"], ["i", "p", "--from", "1,2", "--lake", "0.5"],
                ["i", "p", "--from", "1,2", "--texture", "t", "--painted", "o", "--road-width", "9"],
                ["i", "p", "--from", "1,2", "--texture", "t", "--painted", "o", "--traffic-threshold", "0"]):
        with pytest.raises(SystemExit):
            RT.parse_args(bad)


def test_the_worlds_command_line_takes_routes():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    a = WD.parse_args(base)
    assert a.routes is None and a.sources == [] and a.targets == []
    a = WD.parse_args(base + ["--routes", "pre", "--from", "-5,40", "--from", "3,50", "--to", "-60,35"])
    assert a.region == (-70, 33, 150, 97) and a.routes == "pre"
    assert a.sources == [(-5, 40), (3, 50)] and a.targets == [(-60, 35)]
    for bad in (base + ["--from", "1,40"], base + ["--to", "1,40"], base + ["--routes", "pre"],
                base + ["--routes", "pre", "--from", "80,40"], base + ["--routes", "pre", "--from", "1,40", "--to", "1,32"],
                base + ["--routes", "pre", "--from", "x,y"]):
        with pytest.raises(SystemExit):
            WD.parse_args(bad)
