"""The host side of the regions (gan_heightmaps_amd/regions.py): Areas' validation, the refusals that are made before
the device is touched, the launch sequence on a recording device inside one scratch, max_edges, the Regions' methods and writers
(the GeoJSON parsed back, the SVG parsed as XML), the label makers, Contours.save(regions=...), both command lines.  And the
device code of csrc/regions.hip compiled for the CPU (tests/regions_host/harness.cpp): the same source text the GPU runs -- the
labelling in both forms, the count, the scans, both doublings, the extraction -- bit for bit against tests/regions_ref.py on every
case, once more under the address and undefined-behaviour sanitizers as a stand-alone program.  No device."""
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import regions as RG
from tests import regions_ref as R
from tests.test_render_host import CSRC, ROOT, _compiler

ARRAYS = ("vertex", "ring_offsets", "ring_polygon", "ring_hole", "seed", "label", "cells")


def hand_made(name="nested", origin=(10, -20), areas=None, plane=True):
    e = R.expected(name)
    return RG.report(*(e[k] for k in ARRAYS), RG.Areas() if areas is None else areas, origin, R.case(name).shape,
                     polygon_plane=e["polygon"].copy() if plane else None, rounds=e["rounds"], sweeps=2, form='sweep')


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_areas_validation():
    a = RG.Areas()
    assert (a.min_cells, a.holes) == (1, True) and RG.Areas(np.int64(4), np.bool_(False)) == RG.Areas(4, False) and hash(a) == hash(RG.Areas())
    with pytest.raises(Exception):
        a.min_cells = 3                                                    # frozen
    for kw in (dict(min_cells=0), dict(min_cells=1 << 31), dict(min_cells=2.5), dict(min_cells=True), dict(min_cells=None),
               dict(holes=1), dict(holes=None), dict(holes="no")):
        with pytest.raises(ValueError):
            RG.Areas(**kw)
    assert RG.KEEP == ('polygon',) and RG.FORMS == ('sweep', 'union') and RG.DEFAULT_FORM in RG.FORMS


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    L = R.case("nested")
    for bad in (L.astype(np.float32), L[0], L[None], np.zeros((0, 4), np.int32), "labels", None):
        with pytest.raises(ValueError, match="labels"):
            RG.regions(ops, bad)
    with pytest.raises(ValueError, match="fit int32"):
        RG.regions(ops, L.astype(np.int64) + (1 << 31))
    with pytest.raises(ValueError, match="Areas"):
        RG.regions(ops, L, 4)
    for bad in (3, (1,), (1.5, 2), None):
        with pytest.raises(ValueError, match="origin"):
            RG.regions(ops, L, origin=bad)
    for bad in ("tiled", 0, True):
        with pytest.raises(ValueError, match="form"):
            RG.regions(ops, L, form=bad)
    for bad in (-1, 1.5, 1 << 31, "9"):
        with pytest.raises(ValueError, match="max_edges"):
            RG.regions(ops, L, max_edges=bad)
    with pytest.raises(ValueError, match="keep"):
        RG.regions(ops, L, keep=('component',))
    tex = np.zeros((5, 5, 3), np.uint8)
    for bad in ((1, 2), (1.5, 0, 0), None):
        with pytest.raises(ValueError, match="colour"):
            RG.paint(ops, tex, hand_made(), colour=bad)
    for bad in (-0.1, 1.5, None):
        with pytest.raises(ValueError, match="opacity"):
            RG.paint(ops, tex, hand_made(), opacity=bad)
    with pytest.raises(ValueError, match="outline"):
        RG.paint(ops, tex, hand_made(), outline=1)
    with pytest.raises(ValueError, match="Regions"):
        RG.paint(ops, tex, L)


# ---- the launch sequence ------------------------------------------------------------------------------------------------------------
def recording_ops(name, sweeps=3):
    """a recording device whose extraction answers with the reference's arrays of a case"""
    from tests.fake_device import RecordingOps
    from tests.test_contour_host import Counting
    e = R.expected(name)

    class Ops(RecordingOps):
        def regions_workspace(self, H, W):
            return 1000 + 16 * H * W

        def regions_trace_bytes(self, edges):
            return 500 + 60 * edges

        def regions_label(self, *args):
            self.calls.append(("regions_label", args, {}))
            return sweeps

        def regions_count(self, *args):
            self.calls.append(("regions_count", args, {}))
            return e["edges"], e["polygons"]

        def regions_trace(self, *args):
            self.calls.append(("regions_trace", args, {}))
            return e["rings"], e["vertices"], e["rounds"]

        def regions_extract(self, *args):
            self.calls.append(("regions_extract", args, {}))
            for ptr, k in zip(args[12:19], ARRAYS):
                self.dev._vals[ptr] = e[k]
            if args[19] is not None:
                self.dev._vals[args[19]] = e["polygon"].ravel()

    return Ops(Counting())


SEQUENCE = ["regions_label", "regions_count", "regions_trace", "regions_extract"]


def test_regions_sends_its_launches_inside_one_scratch():
    e, L = R.expected("nested"), R.case("nested")
    ops = recording_ops("nested")
    got = RG.regions(ops, L, origin=(100, -10), form='union', keep=('polygon',), max_edges=60)
    assert [c[0] for c in ops.calls] == SEQUENCE and ops.dev.live == 0
    la, co, tr, ex = (c[1] for c in ops.calls)
    d_l, d_c, d_w = la[0], la[5], la[7]
    assert la[1:5] == (5, 5, 5, 1) and la[6] == 5 and len({d_l, d_c, d_w}) == 3
    assert co == (d_l, 5, d_c, 5, 5, 5, d_w, 60)
    d_t = tr[3]
    assert tr == (5, 5, d_w, d_t, 52, 3)
    assert ex[:12] == (d_l, 5, d_c, 5, 5, 5, d_w, d_t, 52, 3, 5, 20) and len(set(ex[12:20])) == 8 and ex[20] == 5
    # labels, component, the workspace, the per-edge buffers, the seven arrays, the polygon plane
    assert ops.dev.sizes == [100, 100, 1000 + 16 * 25, 500 + 60 * 52, 4 * 20, 8 * 6, 4 * 5, 16, 16, 16, 16, 100]              # an array gets 16 bytes at least
    assert got.shape == (5, 5) and got.origin == (100, -10) and (got.rounds, got.sweeps, got.form) == (e["rounds"], 3, 'union')
    assert len(got) == 3 and np.array_equal(got.vertex, e["vertex"]) and np.array_equal(got.polygon_plane, e["polygon"])
    assert "3 polygons with 2 holes, 20 vertices" in repr(got)
    # the default: no limit on the edges, no polygon plane, the default form
    ops = recording_ops("nested")
    got = RG.regions(ops, L)
    assert ops.calls[1][1][7] == (1 << 31) - 1 and ops.calls[0][1][4] == RG.FORMS.index(RG.DEFAULT_FORM) and len(ops.dev.sizes) == 11
    assert ops.calls[3][1][19] is None and got.polygon_plane is None and ops.dev.live == 0
    # a plane without a region: the labelling says so, and nothing is launched after it
    ops = recording_ops("empty", sweeps=0)
    got = RG.regions(ops, R.case("empty"), keep='polygon')
    assert [c[0] for c in ops.calls] == SEQUENCE[:1] and ops.dev.live == 0 and len(ops.dev.sizes) == 3
    assert len(got) == 0 and got.ring_offsets.tolist() == [0] and got.points.shape == (0, 2) and (got.polygon_plane == -1).all()
    assert got.largest(3) == [] and not got.raster().any() and got.features() == [] and got.sweeps == 0


def test_the_paint_goes_through_the_hydrologys_kernel():
    from tests.fake_device import FakeDevice, RecordingOps
    sent = []

    class Dev(FakeDevice):
        def h2d(self, ptr, arr):
            sent.append(np.array(arr))

    ops = RecordingOps(Dev())
    rg = hand_made("pinch")
    out = RG.paint(ops, np.zeros((4, 4, 3), np.uint8), rg, (1.0, 0.0, 0.0), 0.5, True)
    assert [c[0] for c in ops.calls] == ["hydrology_paint"] and out.shape == (4, 4, 3) and out.dtype == np.uint8
    call = ops.calls[0][1]
    assert call[12] == 1 and call[13] == 0                                 # a mark of 1 is the threshold; no width
    marks = [a for a in sent if a.dtype == np.uint32][0]
    assert np.array_equal(marks.reshape(4, 4), rg.raster(True))
    with pytest.raises(ValueError, match="differ in size"):
        RG.paint(ops, np.zeros((4, 5), np.float32), rg)


# ---- the methods and the writers on a hand-made Regions ------------------------------------------------------------------------------
def test_regions_methods():
    rg = hand_made()
    assert len(rg) == 3 and rg.shape == (5, 5) and rg.origin == (10, -20) and rg.points.dtype == np.int64 and rg.points.shape == (20, 2)
    assert rg.label.tolist() == [0, 1, 0] and rg.cells.tolist() == [16, 8, 1] and rg.seed.tolist() == [0, 6, 12] and rg.hole.tolist() == [0, 1, 0, 1, 0]
    assert rg.rings_of(0) == [0, 1] and rg.rings_of(1) == [2, 3] and rg.rings_of(2) == [4]
    assert rg.ring(0).tolist() == [[10, -20], [10, -15], [15, -15], [15, -20]]              # clockwise on screen
    assert rg.ring(1).tolist() == [[11, -19], [14, -19], [14, -16], [11, -16]]              # a hole runs the other way
    assert [r.tolist() for r in rg.polygon(2)] == [[[12, -18], [12, -17], [13, -17], [13, -18]]]
    assert rg.bbox.tolist() == [[10, -20, 15, -15], [11, -19, 14, -16], [12, -18, 13, -17]] and rg.perimeter.tolist() == [32, 16, 4]
    assert rg.at(10, -20) == 0 and rg.at(11, -19) == 1 and rg.at(12, -18) == 2 and rg.largest(2) == [0, 1] and rg.largest(0) == []
    assert (rg.raster() == 1).all() and rg.raster().dtype == np.uint32 and (rg.raster(True) == 1).all()
    for bad in (3, -1, 1.0, None):
        with pytest.raises(ValueError, match="polygon"):
            rg.rings_of(bad)
    for bad in ((9, -20), (10, -14), (10.0, -20)):
        with pytest.raises(ValueError, match="outside"):
            rg.at(*bad)
    with pytest.raises(ValueError, match="keep"):
        hand_made(plane=False).at(10, -20)
    with pytest.raises(ValueError, match="ring"):
        rg.ring(5)
    # min_cells drops polygons and renumbers; holes=False drops the hole rings, and the raster fills them
    cut = hand_made(areas=RG.Areas(2, False), origin=(0, 0))
    assert len(cut) == 2 and cut.cells.tolist() == [16, 8] and cut.hole.tolist() == [0, 0] and cut.ring_polygon.tolist() == [0, 1]
    assert cut.ring_offsets.tolist() == [0, 4, 8] and cut.perimeter.tolist() == [20, 12] and cut.areas == RG.Areas(2, False)
    assert cut.polygon_plane.tolist()[2] == [0, 1, -1, 1, 0] and (cut.raster() == 1).all()
    big = hand_made(areas=RG.Areas(9), origin=(0, 0))
    assert len(big) == 1 and big.hole.tolist() == [0, 1] and big.raster().tolist()[2] == [1, 0, 0, 0, 1] and big.raster(True).sum() == 16
    # the raster of every reported polygon is the plane's regions; an outline lies on cells with a boundary side
    for name in ("random3", "bands37", "hole_pinch", "serpentine", "land96"):
        L = R.case(name)
        r = hand_made(name, (3, -4))
        assert np.array_equal(r.raster(), (L >= 0).astype(np.uint32)), name
        edge = np.array([[any(R.is_edge(L, y, x, s) for s in range(4)) for x in range(L.shape[1])] for y in range(L.shape[0])])
        assert np.array_equal(r.raster(True), edge.astype(np.uint32)), name
        assert r.perimeter.sum() == R.expected(name)["edges"]


def test_the_writers(tmp_path):
    rg = hand_made()
    rg.save(str(tmp_path / "r.npz"))
    z = np.load(str(tmp_path / "r.npz"))
    for k in ("vertex", "ring_offsets", "points", "ring_polygon", "hole", "seed", "label", "cells", "bbox", "perimeter", "polygon_plane"):
        assert np.array_equal(z[k], getattr(rg, k)) and z[k].dtype == getattr(rg, k).dtype
    assert z["origin"].tolist() == [10, -20] and z["shape"].tolist() == [5, 5] and z["areas"].tolist() == [1, 1]
    rg.save(str(tmp_path / "r.geojson"))
    g = json.load(open(str(tmp_path / "r.geojson")))
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 3 and g["features"] == rg.features()
    f = g["features"][1]
    assert f["geometry"] == {"type": "Polygon", "coordinates": [[[-19, 11], [-16, 11], [-16, 14], [-19, 14], [-19, 11]],
                                                               [[-17, 12], [-18, 12], [-18, 13], [-17, 13], [-17, 12]]]}
    assert f["properties"] == dict(label=1, cells=8, holes=1) and g["features"][2]["properties"] == dict(label=0, cells=1, holes=0)
    for feat in g["features"]:                                            # coordinates [col, row]: the outer ring counter-clockwise in
        for i, ring in enumerate(feat["geometry"]["coordinates"]):       # (x, y up), as GeoJSON wants it -- clockwise on screen
            a2 = sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:]))
            assert ring[0] == ring[-1] and (a2 > 0) == (i == 0)
    tex = np.arange(75, dtype=np.uint8).reshape(5, 5, 3)
    rg.save(str(tmp_path / "r.svg"), texture=tex)
    root = ET.parse(str(tmp_path / "r.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    paths = root.findall(ns + "path")
    assert root.get("viewBox") == "-20 10 5 5" and len(paths) == 3 and all(p.get("class") == "region" for p in paths)
    assert all(p.get("fill-rule") == "evenodd" for p in paths) and [p.get("data-cells") for p in paths] == ["16", "8", "1"]
    assert paths[0].get("d") == "M-20 10 L-15 10 L-15 15 L-20 15 Z M-19 11 L-19 14 L-16 14 L-16 11 Z"
    img = root.findall(ns + "image")
    assert len(img) == 1 and (img[0].get("x"), img[0].get("y"), img[0].get("width"), img[0].get("height")) == ("-20", "10", "5", "5")
    rg.save(str(tmp_path / "s.svg"))
    assert ET.parse(str(tmp_path / "s.svg")).getroot().findall(ns + "image") == []
    with pytest.raises(ValueError, match="size"):
        rg.save(str(tmp_path / "t.svg"), texture=tex[:4])
    with pytest.raises(ValueError, match="npz, .svg or .geojson"):
        rg.save(str(tmp_path / "r.csv"))


# ---- the label planes ------------------------------------------------------------------------------------------------------------------
def test_the_label_makers():
    from gan_heightmaps_amd import route as RT
    from gan_heightmaps_amd import viewshed as VS
    from gan_heightmaps_amd.contour import Levels
    depth = np.array([[0, 0.5, 0.001], [0.25, 0, 0]], np.float32)
    basin = np.array([[0, 0, 5], [0, 5, 5]], np.int32)
    hydro = HY.Hydrology((2, 3), 0, 0, True, depth=depth, basin=basin)
    assert RG.lakes(hydro).tolist() == [[-1, 0, -1], [0, -1, -1]] and RG.lakes(hydro).dtype == np.int32
    assert RG.lakes(hydro, 0).tolist() == [[-1, 0, 0], [0, -1, -1]] and RG.basins(hydro).tolist() == basin.tolist()
    for bad in (depth, None, HY.Hydrology((2, 3), 0, 0, True, basin=basin)):
        with pytest.raises(ValueError, match="kept 'depth'"):
            RG.lakes(bad)
    with pytest.raises(ValueError, match="lake_min_depth"):
        RG.lakes(hydro, -1)
    with pytest.raises(ValueError, match="kept 'basin'"):
        RG.basins(HY.Hydrology((2, 3), 0, 0, True, depth=depth))
    with pytest.raises(ValueError, match="CostField"):
        RG.territories(basin)
    with pytest.raises(ValueError, match="Viewshed"):
        RG.covered(basin)
    count = np.array([[0, 2, 1], [0, 0, 3]], np.uint32)
    vs = VS.Viewshed(count, None, np.zeros((1, 4), np.int32), (0, 0), VS.Sight(), 'plain')
    assert RG.covered(vs).tolist() == [[-1, 0, 0], [-1, -1, 0]] and RG.covered(vs, hidden=True).tolist() == [[0, -1, -1], [0, 0, -1]]
    with pytest.raises(ValueError, match="hidden"):
        RG.covered(vs, hidden=1)
    # land and bands: the viewshed's quantisation, zq = rint(h * 64 * 256)
    h = np.array([[0.0, 0.25, 0.5], [0.5 + 1 / 16384, 0.75, 1.0]], np.float32)
    assert RG.land(h, 0.5).tolist() == [[-1, -1, -1], [0, 0, 0]] and RG.land((h * 255).astype(np.uint8), 0.5).tolist() == [[-1, -1, -1], [-1, 0, 0]]
    assert RG.land(h, 0.5, height_scale=1.0).tolist() == [[-1, -1, -1], [-1, 0, 0]]         # 1/16384 is below 1/256 cell there
    for bad in (-0.1, 1.5, None):
        with pytest.raises(ValueError, match="sea_level"):
            RG.land(h, bad)
    with pytest.raises(ValueError, match="height_scale"):
        RG.land(h, 0.5, height_scale=0)
    with pytest.raises(ValueError):
        RG.land(h * 2, 0.5)
    # levels at 0, 16, 32, 48, 64 cells: the number of them strictly below a cell
    assert RG.bands(h, Levels(16.0)).tolist() == [[0, 1, 2], [3, 3, 4]]
    assert RG.bands(h, Levels(16.0, 16.0)).tolist() == [[0, 0, 1], [2, 2, 3]] and RG.bands(h, Levels(16.0, 0.0, 2)).tolist() == [[0, 1, 2], [2, 2, 2]]
    assert RG.bands(h).dtype == np.int32 and RG.bands(h).max() == 16
    with pytest.raises(ValueError, match="Levels"):
        RG.bands(h, 16.0)
    # the bands' borders are the contours' lines: a cell's band is the count of the levels below it, as tests/regions_ref.py has it
    from tests.contour_ref import heights
    assert np.array_equal(RG.bands(heights(37, 53, 3), Levels(8.0)), R.case("bands37"))


def test_territories_of_a_cost_field():
    from gan_heightmaps_amd import route as RT
    t = np.array([[0, 0, -1], [1, 1, -1]], np.int32)
    cf = RT.CostField((2, 3), sources=((0, 0), (1, 0)), territory=t)
    assert cf.territory is t and RG.territories(cf).tolist() == t.tolist() and RG.territories(cf).dtype == np.int32
    e = R.definition(RG.territories(cf))                                  # the unreached column is no region
    assert e["polygons"] == 2 and e["cells"].tolist() == [2, 2] and e["label"].tolist() == [0, 1]
    with pytest.raises(ValueError, match="kept 'territory'"):
        RG.territories(RT.CostField((2, 3), sources=((0, 0),), cost=np.zeros((2, 3), np.uint32)))


# ---- the contour sheet -------------------------------------------------------------------------------------------------------------------
def test_contours_save_takes_the_regions(tmp_path):
    from tests.test_peaks_host import hand_made as spot_heights, sheet
    from tests.test_rivers_host import blue_lines
    c, p, rv = sheet(), spot_heights(), blue_lines()
    L = np.array([[0, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, -1, -1, 0], [0, 0, 0, 0, 0, 0, 0]], np.int32)
    e = R.definition(L)
    rg = RG.report(*(e[k] for k in ARRAYS), RG.Areas(), (10, -20), (3, 7))
    # without regions every file stays byte for byte what it is today
    c.save(str(tmp_path / "a.svg"), regions=None)
    assert open(str(tmp_path / "a.svg")).read() == c._svg(None)
    c.save(str(tmp_path / "a.geojson"))
    assert open(str(tmp_path / "a.geojson")).read() == json.dumps(c._geojson())
    c.save(str(tmp_path / "b.svg"), peaks=p, rivers=rv)
    plain = open(str(tmp_path / "b.svg")).read()
    assert plain == c._svg(None)[:-len("</svg>\n")] + rv._svg_paths() + c._svg_peaks(p) + "</svg>\n"
    c.save(str(tmp_path / "b.geojson"), peaks=p, rivers=rv)
    assert json.load(open(str(tmp_path / "b.geojson")))["features"] == c._geojson()["features"] + rv.features() + p.features()
    tex = np.zeros((3, 7), np.uint8)
    c.save(str(tmp_path / "t.svg"), texture=tex)
    assert open(str(tmp_path / "t.svg")).read() == c._svg(tex)
    # with them the polygons lie beneath the lines: after the texture, before the first line
    c.save(str(tmp_path / "c.svg"), texture=tex, peaks=p, rivers=rv, regions=rg)
    root = ET.parse(str(tmp_path / "c.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    kinds = [(el.tag[len(ns):], el.get("class")) for el in root]
    assert kinds[:2] == [("image", None), ("g", None)] and kinds[2][0] == "path" and kinds[2][1] in ("line", "index")
    assert kinds[3:] == [("path", "river"), ("circle", "peak"), ("text", "peak"), ("circle", "peak"), ("text", "peak")]
    group = root.findall(ns + "g")[0]
    assert group.get("transform") == "translate(-0.5 -0.5)" and [el.get("class") for el in group] == ["region"] * len(rg) and len(rg) == 2
    assert group[0].get("d") == "M-20 10 L-13 10 L-13 13 L-20 13 Z M-19 11 L-19 12 L-17 12 L-17 11 Z M-16 11 L-16 12 L-14 12 L-14 11 Z"
    text = open(str(tmp_path / "c.svg")).read()
    cut = text.index("<g "), text.index("</g>\n") + len("</g>\n")
    c.save(str(tmp_path / "d.svg"), texture=tex, peaks=p, rivers=rv)
    assert text[:cut[0]] + text[cut[1]:] == open(str(tmp_path / "d.svg")).read()
    c.save(str(tmp_path / "e.svg"), regions=rg)
    assert [el.tag[len(ns):] for el in ET.parse(str(tmp_path / "e.svg")).getroot()] == ["g", "path"]
    c.save(str(tmp_path / "c.geojson"), peaks=p, rivers=rv, regions=rg)
    g = json.load(open(str(tmp_path / "c.geojson")))
    assert [f["geometry"]["type"] for f in g["features"]] == ["Polygon", "Polygon", "LineString", "LineString", "Point", "Point"]
    assert g["features"][:2] == rg.features() and g["features"][2:3] == c._geojson()["features"]
    for bad in (RG.report(*(e[k] for k in ARRAYS), RG.Areas(), (0, 0), (3, 7)), "regions", hand_made()):
        with pytest.raises(ValueError, match="Regions of the contours' plane"):
            c.save(str(tmp_path / "f.svg"), regions=bad)
    with pytest.raises(ValueError, match="npz"):
        c.save(str(tmp_path / "f.npz"), regions=rg)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    from gan_heightmaps_amd.contour import Levels
    a = RG.parse_args(["in.png", "out.geojson", "--lakes"])
    assert (a.input, a.output, a.of, a.areas, a.texture, a.painted, a.form, a.outline, a.opacity) == (
        "in.png", "out.geojson", "lakes", RG.Areas(), None, None, None, False, 0.6)
    a = RG.parse_args(["i.npy", "o.svg", "--bands", "--interval", "8", "--base", "2", "--min-cells", "5", "--no-holes", "--texture", "t.png",
                       "--painted", "p.png", "--colour", "0.5,0.25,0", "--opacity", "0.5", "--outline", "--union"])
    assert a.of == "bands" and a.levels == Levels(8.0, 2.0) and a.areas == RG.Areas(5, False) and (a.texture, a.painted, a.colour, a.opacity,
                                                                                                  a.outline, a.form) == ("t.png", "p.png", (0.5, 0.25, 0.0), 0.5, True, "union")
    a = RG.parse_args(["i", "o.NPZ", "--land", "0.25", "--sweep"])
    assert (a.of, a.sea, a.form) == ("land", 0.25, "sweep") and RG.parse_args(["i", "o.svg", "--basins"]).of == "basins"
    assert RG.parse_args(["l.npy", "o.svg", "--labels"]).of == "labels"
    for bad in (["i"], ["i", "o.svg"], ["i", "o.csv", "--lakes"], ["i", "o.svg", "--lakes", "--basins"], ["i", "o.svg", "--land"],
                ["i", "o.svg", "--land", "1.5"], ["i", "o.svg", "--land", "x"], ["i", "o.svg", "--lakes", "--interval", "8"],
                ["i", "o.svg", "--bands", "--interval", "0"], ["i", "o.svg", "--lakes", "--min-cells", "0"],
                ["i", "o.svg", "--lakes", "--painted", "p.png"], ["i", "o.svg", "--lakes", "--texture", "t.png"], ["i", "o.svg", "--lakes", "--outline"],
                ["i", "o.svg", "--lakes", "--sweep", "--union"], ["i", "o.svg", "--lakes", "--texture", "t", "--painted", "p", "--colour", "2,0,0"],
                ["i", "o.svg", "--lakes", "--texture", "t", "--painted", "p", "--opacity", "2"]):
        with pytest.raises(SystemExit):
            RG.parse_args(bad)


def test_the_worlds_command_line_takes_regions():
    from gan_heightmaps_amd import world as WD
    from gan_heightmaps_amd.contour import Levels
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    assert WD.parse_args(base).regions is None
    a = WD.parse_args(base + ["--regions", "water.geojson", "--of", "lakes", "--min-cells", "8", "--no-holes"])
    assert (a.regions, a.of, a.areas, a.sea_level) == ("water.geojson", "lakes", RG.Areas(8, False), None)
    a = WD.parse_args(base + ["--regions", "land.svg", "--of", "land", "--sea-level", "0.4"])
    assert (a.of, a.sea_level, a.areas) == ("land", 0.4, RG.Areas())
    a = WD.parse_args(base + ["--regions", "b.npz", "--of", "bands", "--interval", "8", "--base", "2"])
    assert a.band_levels == Levels(8.0, 2.0) and a.contours is None
    a = WD.parse_args(base + ["--regions", "b.npz", "--of", "bands", "--contours", "sheet.svg", "--interval", "8", "--rivers", "r.svg"])
    assert (a.regions, a.contours, a.rivers) == ("b.npz", "sheet.svg", "r.svg") and a.levels == Levels(8.0) == a.band_levels
    for bad in (["--regions", "w.csv", "--of", "lakes"], ["--regions", "w.svg"], ["--of", "lakes"], ["--min-cells", "4"], ["--no-holes"],
                ["--sea-level", "0.5"], ["--regions", "w.svg", "--of", "land"], ["--regions", "w.svg", "--of", "lakes", "--sea-level", "0.5"],
                ["--regions", "w.svg", "--of", "land", "--sea-level", "2"], ["--regions", "w.svg", "--of", "seas"],
                ["--regions", "w.svg", "--of", "lakes", "--min-cells", "0"], ["--regions", "w.svg", "--of", "lakes", "--interval", "8"],
                ["--interval", "8"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "regions.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "regions.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
           '-DREGIONS_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "regions_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("regions_host")
    exe, r = _build(d, "regions_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_plane(harness, L, form):
    """-> dict of everything the harness gives; the labels go in with rows of W + 3 cells whose padding repeats the row's last label,
    component and polygon come back in rows of W + 2 cells whose padding must be untouched"""
    d, exe = harness
    H, W = L.shape
    wide = np.empty((H, W + 3), np.int32)
    wide[:, :W] = L
    wide[:, W:] = L[:, -1:]
    (d / "in.bin").write_bytes(wide.tobytes())
    args = ["run", H, W, W + 3, W + 2, RG.FORMS.index(form), d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    E, P, Rn, V, rounds, sweeps = [int(v) for v in np.frombuffer(raw[:64], np.int64)][:6]
    at = [64]

    def take(dtype, n):
        a = np.frombuffer(raw[at[0]:at[0] + n * np.dtype(dtype).itemsize], dtype)
        at[0] += a.nbytes
        return a

    planes = [take(np.int32, H * (W + 2)).reshape(H, W + 2) for _ in range(2)]
    for plane in planes:
        assert (plane[:, W:].view(np.uint8) == 0xAB).all(), "cells beyond a row's width were written"
    got = dict(component=np.ascontiguousarray(planes[0][:, :W]), polygon=np.ascontiguousarray(planes[1][:, :W]), vertex=take(np.int32, V),
               ring_offsets=take(np.int64, Rn + 1), ring_polygon=take(np.int32, Rn), ring_hole=take(np.uint8, Rn), seed=take(np.int32, P),
               label=take(np.int32, P), cells=take(np.uint32, P), edges=E, polygons=P, rings=Rn, vertices=V, rounds=rounds, sweeps=sweeps)
    assert at[0] == len(raw)
    return got


KEYS = ("component", "polygon") + ARRAYS
COUNTS = ("edges", "polygons", "rings", "vertices", "rounds")


def check_case(harness, name, form):
    want = R.expected(name)
    got = run_plane(harness, R.case(name), form)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, form, k)
    for k in COUNTS:
        assert got[k] == want[k], (name, form, k)
    return got


@pytest.mark.parametrize("form", RG.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_on_the_host_build(harness, name, form):
    got = check_case(harness, name, form)
    if name in R.TABLE:
        assert (got["edges"], got["rings"], got["polygons"], got["vertices"]) == R.TABLE[name][:3] + R.TABLE[name][4:]
    if name == "serpentine":
        assert got["rounds"] == 11 and (got["sweeps"] >= 2 if form == 'sweep' else got["sweeps"] == 1)
    if name == "bands96":
        assert got["rounds"] == 12
    if name == "checker96":                                                # 145 blocks of edges in a scan, 37 of cells
        assert got["edges"] == 4 * 96 * 96 > 256 * 32 * 4


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, run as a child process: an index past a plane, a tile's
    slots, a per-edge buffer or a dense array and signed overflow in the kernels' arithmetic end it"""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    # only a compiler that cannot build and run an empty program with the sanitizers is a reason to skip
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([_compiler(), "-x", "c++"] + flags + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")],
                           capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "empty")]).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + probe.stderr[-300:])
    exe, r = _build(tmp_path, "regions_host_san", flags)
    assert r.returncode == 0, r.stderr[-3000:]
    h = (tmp_path, exe)
    for name in sorted(R.CASES):
        for form in RG.FORMS:
            check_case(h, name, form)
