"""The host side of the rivers (gan_heightmaps_amd/rivers.py): Network's validation, the refusals that are made before
the device is touched, the launch sequence on a recording device inside one scratch, the max_reaches refusal, the Rivers' methods
and writers, the min_order filter, Contours.save(rivers=...), both command lines.  And the device code of csrc/rivers.hip compiled
for the CPU (tests/rivers_host/harness.cpp): the same source text the GPU runs -- the count, the scans, the doubling rounds in both
forms, the tails, the extraction -- and ghm_rivers_order's body, bit for bit against tests/rivers_ref.py on the cases of the device
tests, once more under the address and undefined-behaviour sanitizers.  No device."""
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import rivers as RV
from tests import rivers_ref as R
from tests.test_render_host import CSRC, ROOT, _compiler


def hydro_of(name, **planes):
    d, A, T = R.planes(name)
    return HY.Hydrology(d.shape, (0, 0), 0, True, direction=d, accumulation=A, **planes), T


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_network_validation():
    n = RV.Network()
    assert (n.river_threshold, n.min_order, n.lake_min_depth) == (256, 1, 1.0 / 512)
    assert RV.Network(np.int64(8), np.int32(2), np.float32(0.5)) == RV.Network(8, 2, 0.5) and hash(n) == hash(RV.Network())
    with pytest.raises(Exception):
        n.min_order = 3                                                    # frozen
    for kw in (dict(river_threshold=0), dict(river_threshold=1 << 32), dict(river_threshold=2.5), dict(river_threshold=True),
               dict(river_threshold=None), dict(min_order=0), dict(min_order=65), dict(min_order=1.5), dict(min_order=True),
               dict(min_order="2"), dict(lake_min_depth=-1), dict(lake_min_depth=float("nan")), dict(lake_min_depth=float("inf")),
               dict(lake_min_depth=None)):
        with pytest.raises(ValueError):
            RV.Network(**kw)
    assert RV.KEEP == ('kind',) and RV.FORMS == ('plain', 'list') and RV.DEFAULT_FORM in RV.FORMS
    assert (RV.STREAM, RV.SOURCE, RV.CONFLUENCE, RV.MOUTH) == (R.STREAM, R.SOURCE, R.CONFLUENCE, R.MOUTH)


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    hydro, _ = hydro_of("star7")
    d, A, _ = R.planes("star7")
    for bad in (d, None, HY.Hydrology(d.shape, (0, 0), 0, True, direction=d), HY.Hydrology(d.shape, (0, 0), 0, True, accumulation=A)):
        with pytest.raises(ValueError, match="kept 'direction' and 'accumulation'"):
            RV.rivers(ops, bad)
    with pytest.raises(ValueError, match="4 x 3"):
        RV.rivers(ops, HY.Hydrology(d.shape, (0, 0), 0, True, direction=d, accumulation=A[:3]))
    with pytest.raises(ValueError, match="Network"):
        RV.rivers(ops, hydro, 256)
    for bad in (3, (1,), (1.5, 2), None):
        with pytest.raises(ValueError, match="origin"):
            RV.rivers(ops, hydro, origin=bad)
    for bad in ("tiled", 0, True):
        with pytest.raises(ValueError, match="form"):
            RV.rivers(ops, hydro, form=bad)
    for bad in (-1, 1.5, None, 1 << 31):
        with pytest.raises(ValueError, match="max_reaches"):
            RV.rivers(ops, hydro, max_reaches=bad)
    with pytest.raises(ValueError, match="keep"):
        RV.rivers(ops, hydro, keep=('area',))
    tex = np.zeros((4, 3, 3), np.uint8)
    for bad in ((1, 2), (1.5, 0, 0), None):
        with pytest.raises(ValueError, match="colour"):
            RV.paint(ops, tex, hand_made(), colour=bad)
    for bad in (-1, 5, 1.0):
        with pytest.raises(ValueError, match="width"):
            RV.paint(ops, tex, hand_made(), width=bad)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match="min_order"):
            RV.paint(ops, tex, hand_made(), min_order=bad)
    for bad in (-0.1, 1.5, None):
        with pytest.raises(ValueError, match="opacity"):
            RV.paint(ops, tex, hand_made(), opacity=bad)
    with pytest.raises(ValueError, match="Rivers"):
        RV.paint(ops, tex, hydro)


# ---- the launch sequence ------------------------------------------------------------------------------------------------------------
def recording_ops(name, reaches=None):
    """a recording device whose count and extraction answer with the reference's arrays of a case"""
    from tests.fake_device import RecordingOps
    from tests.test_contour_host import Counting
    e = R.expected(name)

    class Ops(RecordingOps):
        def rivers_workspace(self, H, W):
            return 1000 + 32 * H * W

        def rivers_list_bytes(self, cells):
            return 500 + 20 * cells

        def rivers_count(self, *args):
            self.calls.append(("rivers_count", args, {}))
            return (e["cells"], e["reaches"] if reaches is None else reaches, e["sources"], e["confluences"], e["mouths"], e["isolated"])

        def rivers_trace(self, *args):
            self.calls.append(("rivers_trace", args, {}))
            return len(e["vertex"]), 3

        def rivers_extract(self, *args):
            self.calls.append(("rivers_extract", args, {}))
            for ptr, arr in zip(args[-3:], (e["vertex"], e["offsets"], e["downstream"])):
                self.dev._vals[ptr] = arr

        def rivers_order(self, downstream, area):
            self.calls.append(("rivers_order", (len(downstream), area.tolist()), {}))
            return e["order"], e["magnitude"], e["main"]

    return Ops(Counting())


SEQUENCE = ["rivers_count", "rivers_trace", "rivers_extract", "rivers_order"]


def test_rivers_sends_its_launches_inside_one_scratch():
    e = R.expected("star7")
    hydro, T = hydro_of("star7")
    ops = recording_ops("star7")
    got = RV.rivers(ops, hydro, RV.Network(T), origin=(100, -10), form='list', keep=('kind',))
    assert [c[0] for c in ops.calls] == SEQUENCE and ops.dev.live == 0
    co, tr, ex, od = (c[1] for c in ops.calls)
    assert co[1] == 3 and co[3:7] == (3, 4, 3, T) and co[8] == 3
    d_dir, d_acc, d_kind, d_w = co[0], co[2], co[7], co[9]
    assert tr[:7] == (d_dir, 3, d_kind, 3, 4, 3, 1) and tr[7] == d_w and tr[9:] == (e["cells"], 8)
    d_l = tr[8]
    assert ex[:8] == (d_dir, 3, d_kind, 3, 4, 3, d_w, d_l) and ex[8:11] == (e["cells"], 8, 17) and len(set(ex[11:])) == 3
    assert od == (8, e["area"].tolist())                                   # the areas are the host's, from the planes
    # direction, accumulation, kind, the workspace, the list, then the three arrays
    assert ops.dev.sizes == [12, 48, 12, 1000 + 32 * 12, 500 + 20 * e["cells"], 4 * 17, 8 * 9, 4 * 8]
    assert d_l is not None and len({d_dir, d_acc, d_kind, d_w, d_l}) == 5
    assert got.shape == (4, 3) and got.origin == (100, -10) and got.rounds == 3 and got.form == 'list' and len(got) == 8
    assert (got.sources_count, got.confluences_count, got.mouths_count, got.isolated) == (9, 1, 3, 2)
    assert got.kind.shape == (4, 3) and got.height is None and got.lake is None and "8 reaches of order up to 2" in repr(got)
    assert np.array_equal(got.vertex, e["vertex"]) and np.array_equal(got.order, e["order"])
    # the plain form allocates no list; filled and depth give the heights and the lakes
    ops = recording_ops("star7")
    filled = np.arange(12, dtype=np.float32).reshape(4, 3) / 8
    depth = np.where(np.arange(12).reshape(4, 3) == 7, np.float32(0.5), np.float32(0))
    hydro, T = hydro_of("star7", filled=filled, depth=depth)
    got = RV.rivers(ops, hydro, RV.Network(T, 2), form='plain')
    assert [c[0] for c in ops.calls] == SEQUENCE and ops.dev.live == 0 and len(ops.dev.sizes) == 7
    assert ops.calls[1][1][6] == 0 and ops.calls[1][1][8] is None and got.kind is None
    assert len(got) == 1 and got.vertex.tolist() == [4, 7, 10] and got.downstream.tolist() == [-1]
    assert got.height.tolist() == [0.5, 0.875, 1.25] and got.height.dtype == np.float32 and got.lake.tolist() == [0, 1, 0]
    # nothing to report: every array is empty
    ops = recording_ops("single")
    hydro, T = hydro_of("single")
    got = RV.rivers(ops, hydro, RV.Network(T))
    assert len(got) == 0 and got.isolated == 1 and got.offsets.tolist() == [0] and got.points.shape == (0, 2) and got.length.shape == (0,)
    assert got.sources() == [] and got.mouths() == [] and got.lines() == [] and not got.raster().any() and ops.dev.live == 0
    assert ops.dev.sizes[-3:] == [16, 16, 16]                              # an empty array still gets a pointer


def test_more_reaches_than_max_reaches_are_refused_before_the_trace():
    hydro, T = hydro_of("star7")
    ops = recording_ops("star7", reaches=41)
    with pytest.raises(ValueError, match="41 reaches"):
        RV.rivers(ops, hydro, RV.Network(T), form='list', max_reaches=40)
    assert [c[0] for c in ops.calls] == SEQUENCE[:1] and ops.dev.live == 0
    assert len(ops.dev.sizes) == 4                                         # no list, no array of the extraction
    ops = recording_ops("star7")
    RV.rivers(ops, hydro, RV.Network(T), max_reaches=8)


def test_the_paint_goes_through_the_hydrologys_kernel():
    from tests.fake_device import FakeDevice, RecordingOps
    sent = []

    class Dev(FakeDevice):
        def h2d(self, ptr, arr):
            sent.append(np.array(arr))

    ops = RecordingOps(Dev())
    rv = hand_made()
    out = RV.paint(ops, np.zeros((4, 3, 3), np.uint8), rv, 2, 1, (1.0, 0.0, 0.0))
    assert [c[0] for c in ops.calls] == ["hydrology_paint"] and out.shape == (4, 3, 3) and out.dtype == np.uint8
    call = ops.calls[0][1]
    assert call[12] == 2 and call[13] == 1                                 # min_order is the threshold, then the width
    marks = [a for a in sent if a.dtype == np.uint32][0]
    assert np.array_equal(marks.reshape(4, 3), rv.raster())
    with pytest.raises(ValueError, match="differ in size"):
        RV.paint(ops, np.zeros((4, 4), np.float32), rv)


# ---- the methods and the writers on a hand-made Rivers -------------------------------------------------------------------------------
def hand_made(origin=(10, -20), name="star7", network=None):
    """the eight reaches of the case star7 at ``origin``"""
    e = R.expected(name)
    d, A, T = R.planes(name)
    return RV.report(e["vertex"], e["offsets"], e["downstream"], e["order"], e["magnitude"], e["main"], e["area"],
                     RV.Network(T) if network is None else network, origin, d.shape, rounds=e["rounds"], form='plain',
                     sources_count=e["sources"], confluences_count=e["confluences"], mouths_count=e["mouths"], isolated=e["isolated"])


def test_rivers_methods():
    rv = hand_made()
    assert len(rv) == 8 and rv.shape == (4, 3) and rv.origin == (10, -20) and rv.isolated == 2
    assert rv.points.dtype == np.int64 and rv.points.shape == (17, 2) and rv.offsets.dtype == np.int64
    assert rv.line(4).tolist() == [[11, -19], [12, -19], [13, -19]] and rv.line(0).tolist() == [[10, -20], [11, -19]]
    assert rv.downstream.tolist() == [4, 4, 4, 4, -1, 4, 4, 4] and rv.order.tolist() == [1, 1, 1, 1, 2, 1, 1, 1]
    assert rv.magnitude.tolist() == [1, 1, 1, 1, 7, 1, 1, 1] and rv.main.tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
    assert rv.area.tolist() == [1, 1, 1, 1, 10, 1, 1, 1] and rv.area.dtype == np.uint32
    s2 = np.sqrt(2.0)
    assert rv.length.dtype == np.float64 and rv.length.tolist() == [s2, 1.0, s2, 1.0, 2.0, 1.0, s2, s2]
    assert [i for i, _ in rv.lines()] == list(range(8)) and [i for i, _ in rv.lines(min_order=2)] == [4]
    assert rv.stem(0) == [0, 4] and rv.stem(4) == [4] and rv.tributaries(4) == [0, 1, 2, 3, 5, 6, 7] and rv.tributaries(0) == []
    assert rv.sources() == [(10, -20), (10, -19), (10, -18), (11, -20), (11, -18), (12, -20), (12, -18)]
    assert rv.confluences() == [(11, -19)] and rv.mouths() == [(13, -19)]
    assert rv.raster().tolist() == [[1, 1, 1], [1, 2, 1], [1, 2, 1], [0, 2, 0]] and rv.raster().dtype == np.uint32
    for bad in (8, -1, 1.0, None):
        with pytest.raises(ValueError, match="reach"):
            rv.line(bad)
        with pytest.raises(ValueError, match="reach"):
            rv.stem(bad)
    with pytest.raises(ValueError, match="min_order"):
        rv.lines(min_order=0)
    # a row: one reach whose end is a mouth with one inflow
    row = hand_made((0, 0), "row")
    assert len(row) == 1 and row.length.tolist() == [8.0] and row.area.tolist() == [9] and row.mouths() == [(0, 8)] and row.sources() == [(0, 0)]


def test_min_order_drops_reaches_and_renumbers_downstream():
    name = "noise3_t2"
    e = R.expected(name)
    whole = hand_made((0, 0), name)
    assert len(whole) == e["reaches"] and int(e["order"].max()) >= 3
    for least in (2, 3):
        d, A, T = R.planes(name)
        cut = hand_made((0, 0), name, RV.Network(T, least))
        keep = np.flatnonzero(e["order"] >= least)
        assert 0 < len(cut) == len(keep) < len(whole) and cut.network.min_order == least
        assert np.array_equal(cut.order, e["order"][keep]) and np.array_equal(cut.magnitude, e["magnitude"][keep])
        assert np.array_equal(cut.main, e["main"][keep]) and np.array_equal(cut.area, e["area"][keep])
        for i, r in enumerate(keep):
            assert np.array_equal(cut.line(i), whole.line(int(r)))
            if e["downstream"][r] < 0:
                assert cut.downstream[i] == -1
            else:                                                          # the kept set is closed downstream
                assert keep[cut.downstream[i]] == e["downstream"][r]
                assert np.array_equal(cut.line(int(cut.downstream[i]))[0], cut.line(i)[-1])
        assert cut.offsets[-1] == len(cut.vertex) and cut.downstream.dtype == np.int32 and (cut.sources_count, cut.isolated) == (
            whole.sources_count, whole.isolated)


def test_the_writers(tmp_path):
    rv = hand_made()
    rv.save(str(tmp_path / "r.npz"))
    z = np.load(str(tmp_path / "r.npz"))
    for k in ("vertex", "offsets", "points", "downstream", "order", "magnitude", "main", "area", "length"):
        assert np.array_equal(z[k], getattr(rv, k)) and z[k].dtype == getattr(rv, k).dtype
    assert z["origin"].tolist() == [10, -20] and z["shape"].tolist() == [4, 3] and z["network"].tolist() == [1.0, 1.0, 1.0 / 512]
    assert "height" not in z.files and "lake" not in z.files
    rv.save(str(tmp_path / "r.geojson"))
    g = json.load(open(str(tmp_path / "r.geojson")))
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 8 and g["features"] == rv.features()
    f = g["features"][4]
    assert f["geometry"] == {"type": "LineString", "coordinates": [[-19, 11], [-19, 12], [-19, 13]]}
    assert f["properties"] == dict(order=2, magnitude=7, main=True, area=10, length=2.0, downstream=-1)
    assert g["features"][1]["properties"] == dict(order=1, magnitude=1, main=False, area=1, length=1.0, downstream=4)
    rv.save(str(tmp_path / "r.svg"))
    root = ET.parse(str(tmp_path / "r.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    paths = root.findall(ns + "path")
    assert root.get("viewBox") == "-20 10 2 3" and len(paths) == 8 and all(p.get("class") == "river" for p in paths)
    assert [p.get("data-order") for p in paths] == ["1", "1", "1", "1", "2", "1", "1", "1"]
    assert paths[4].get("d") == "M-19 11 L-19 12 L-19 13" and float(paths[4].get("stroke-width")) > float(paths[0].get("stroke-width"))
    with pytest.raises(ValueError, match="npz, .svg or .geojson"):
        rv.save(str(tmp_path / "r.csv"))


def blue_lines(origin=(10, -20)):
    """a Rivers of the 3 x 7 plane of tests.test_peaks_host.sheet: the middle row flows east, one reach"""
    d = np.full((3, 7), -1, np.int8)
    d[1, :6] = 2
    e = R.definition(d, R.accumulation(d), 2)
    assert e["reaches"] == 1 and e["vertex"].tolist() == [8, 9, 10, 11, 12, 13]
    return RV.report(e["vertex"], e["offsets"], e["downstream"], e["order"], e["magnitude"], e["main"], e["area"], RV.Network(2), origin, (3, 7))


def test_contours_save_takes_the_rivers(tmp_path):
    from tests.test_peaks_host import hand_made as spot_heights, sheet
    c, p, rv = sheet(), spot_heights(), blue_lines()
    # without rivers both files are byte for byte what the untouched _svg and _geojson give
    c.save(str(tmp_path / "a.svg"), rivers=None)
    assert open(str(tmp_path / "a.svg")).read() == c._svg(None)
    c.save(str(tmp_path / "a.geojson"))
    assert open(str(tmp_path / "a.geojson")).read() == json.dumps(c._geojson())
    c.save(str(tmp_path / "b.svg"), peaks=p, rivers=rv)
    text = open(str(tmp_path / "b.svg")).read()
    assert text.startswith(c._svg(None)[:-len("</svg>\n")]) and text.endswith("</svg>\n")
    root = ET.parse(str(tmp_path / "b.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    kinds = [(el.tag[len(ns):], el.get("class")) for el in root]
    assert kinds[0][0] == "path" and kinds[0][1] in ("line", "index")       # the contour, then the river, then the peaks' marks
    assert kinds[1:] == [("path", "river"), ("circle", "peak"), ("text", "peak"), ("circle", "peak"), ("text", "peak")]
    assert root.findall(ns + "path")[1].get("d") == "M-19 11 L-18 11 L-17 11 L-16 11 L-15 11 L-14 11"
    c.save(str(tmp_path / "b.geojson"), peaks=p, rivers=rv)
    g = json.load(open(str(tmp_path / "b.geojson")))
    assert [f["geometry"]["type"] for f in g["features"]] == ["LineString", "LineString", "Point", "Point"]
    assert g["features"][:1] == c._geojson()["features"] and g["features"][1:2] == rv.features() and g["features"][2:] == p.features()
    c.save(str(tmp_path / "c.geojson"), rivers=rv)
    assert json.load(open(str(tmp_path / "c.geojson")))["features"][1:] == rv.features()
    for bad in (blue_lines(origin=(0, 0)), "rivers", hand_made()):
        with pytest.raises(ValueError, match="Rivers of the contours' plane"):
            c.save(str(tmp_path / "d.svg"), rivers=bad)
    with pytest.raises(ValueError, match="npz"):
        c.save(str(tmp_path / "d.npz"), rivers=rv)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = RV.parse_args(["in.png", "out.geojson"])
    assert (a.input, a.output, a.network, a.texture, a.painted, a.form, a.width, a.opacity) == (
        "in.png", "out.geojson", RV.Network(), None, None, None, 0, 0.85)
    a = RV.parse_args(["i.npy", "o.svg", "--river-threshold", "32", "--min-order", "2", "--lake-min-depth", "0.25", "--texture", "t.png",
                       "--painted", "p.png", "--width", "2", "--colour", "0.5,0.25,0", "--opacity", "0.5", "--list"])
    assert a.network == RV.Network(32, 2, 0.25) and (a.texture, a.painted, a.width, a.colour, a.opacity, a.form) == (
        "t.png", "p.png", 2, (0.5, 0.25, 0.0), 0.5, "list")
    assert RV.parse_args(["i", "o.NPZ", "--plain"]).form == "plain"
    for bad in (["i"], ["i", "o.csv"], ["i", "o.svg", "--river-threshold", "0"], ["i", "o.svg", "--river-threshold", "x"],
                ["i", "o.svg", "--min-order", "0"], ["i", "o.svg", "--min-order", "1.5"], ["i", "o.svg", "--lake-min-depth", "-1"],
                ["i", "o.svg", "--painted", "p.png"], ["i", "o.svg", "--texture", "t.png"], ["i", "o.svg", "--plain", "--list"],
                ["i", "o.svg", "--texture", "t", "--painted", "p", "--colour", "2,0,0"],
                ["i", "o.svg", "--texture", "t", "--painted", "p", "--width", "9"],
                ["i", "o.svg", "--texture", "t", "--painted", "p", "--opacity", "2"]):
        with pytest.raises(SystemExit):
            RV.parse_args(bad)


def test_the_worlds_command_line_takes_rivers():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    assert WD.parse_args(base).rivers is None
    a = WD.parse_args(base + ["--rivers", "blue.geojson", "--river-threshold", "64", "--min-order", "2"])
    assert a.rivers == "blue.geojson" and a.network == RV.Network(64, 2)
    assert WD.parse_args(base + ["--rivers", "blue.svg"]).network == RV.Network()
    a = WD.parse_args(base + ["--rivers", "blue.npz", "--contours", "sheet.svg", "--peaks", "tops.csv"])
    assert (a.rivers, a.contours, a.peaks) == ("blue.npz", "sheet.svg", "tops.csv")
    for bad in (["--rivers", "blue.csv"], ["--river-threshold", "64"], ["--min-order", "2"], ["--rivers", "b.svg", "--river-threshold", "0"],
                ["--rivers", "b.svg", "--min-order", "0"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "rivers.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "rivers.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
           '-DRIVERS_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "rivers_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("rivers_host")
    exe, r = _build(d, "rivers_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_planes(harness, direction, A, T, form, want_code=0):
    """-> dict of everything the harness gives; the planes go in with rows of W + 3 cells whose padding points east and is 2^32 - 1
    of area, kind comes back in rows of W + 2 cells whose padding must be untouched"""
    d, exe = harness
    H, W = direction.shape
    wide_a = np.full((H, W + 3), 0xffffffff, np.uint32)
    wide_a[:, :W] = A
    wide_d = np.full((H, W + 3), 2, np.int8)
    wide_d[:, :W] = direction
    (d / "in.bin").write_bytes(wide_a.tobytes() + wide_d.tobytes())
    args = ["run", H, W, W + 3, W + 2, T, RV.FORMS.index(form), d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == want_code, (r.returncode, r.stderr[-3000:])
    if want_code:
        return None
    raw = (d / "out.bin").read_bytes()
    head = [int(v) for v in np.frombuffer(raw[:64], np.int64)]
    cells, Rn, sources, confluences, mouths, isolated, V, rounds = head
    at = [64]

    def take(dtype, n):
        a = np.frombuffer(raw[at[0]:at[0] + n * np.dtype(dtype).itemsize], dtype)
        at[0] += a.nbytes
        return a

    kind = take(np.uint8, H * (W + 2)).reshape(H, W + 2)
    assert (kind[:, W:] == 0xAB).all(), "cells beyond a row's width were written"
    got = dict(kind=np.ascontiguousarray(kind[:, :W]), vertex=take(np.int32, V), offsets=take(np.int64, Rn + 1),
               downstream=take(np.int32, Rn), area=take(np.uint32, Rn), order=take(np.int32, Rn), magnitude=take(np.int32, Rn),
               main=take(np.uint8, Rn), cells=cells, reaches=Rn, sources=sources, confluences=confluences, mouths=mouths,
               isolated=isolated, rounds=rounds)
    assert at[0] == len(raw)
    return got


KEYS = ("kind", "vertex", "offsets", "downstream", "area", "order", "magnitude", "main")
COUNTS = ("cells", "reaches", "sources", "confluences", "mouths", "isolated", "rounds")


def check_case(harness, name, form):
    want = R.expected(name)
    got = run_planes(harness, *R.planes(name), form)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, form, k)
    for k in COUNTS:
        assert got[k] == want[k], (name, form, k)
    return got


@pytest.mark.parametrize("form", RV.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_on_the_host_build(harness, name, form):
    got = check_case(harness, name, form)
    if name == "serpentine_t8":
        assert got["rounds"] == 9 and len(got["vertex"]) == 506
    if name == "comb":
        assert got["reaches"] == 1799 and got["rounds"] == 0
    # the host's areas, as gan_heightmaps_amd/rivers.py takes them from the planes, are the definition's
    d, A, T = R.planes(name)
    assert np.array_equal(RV.reach_areas(got["vertex"], got["offsets"], got["downstream"], d, A), R.expected(name)["area"])


def test_the_harness_refuses_what_the_definition_refuses(harness):
    d, A, T = R.planes("row")
    for at, v, code in (((0, 3), 9, 7), ((0, 3), -2, 7), ((0, 8), 2, 8), ((0, 0), 6, 8)):
        bad = d.copy()
        bad[at] = v
        run_planes(harness, bad, A, T, 'plain', want_code=code)
    bad = A.copy()
    bad[0, 5] = 5
    run_planes(harness, d, bad, T, 'plain', want_code=9)
    assert run_planes(harness, d, bad, 6, 'list')["reaches"] == 1


def test_the_order_refuses_what_is_no_forest(harness):
    d, exe = harness

    def order(downstream, area):
        (d / "o.bin").write_bytes(np.asarray(downstream, np.int32).tobytes() + np.asarray(area, np.uint32).tobytes())
        return subprocess.run([str(exe), "order", str(len(downstream)), str(d / "o.bin"), str(d / "o.out")]).returncode

    assert order([], []) == 0 and order([1, -1], [1, 2]) == 0
    assert order([2, -1], [1, 1]) == 21 and order([-2, -1], [1, 1]) == 21          # outside [-1, R)
    assert order([0], [1]) == 22 and order([1, 1], [1, 1]) == 22                    # its own downstream
    assert order([1, 0], [1, 1]) == 23 and order([1, 2, 0, -1], [1, 1, 1, 1]) == 23          # a cycle
    # reach numbers are not topological: a chain numbered against the flow
    assert order([-1, 0, 1, 2, 2], [5, 4, 3, 1, 1]) == 0
    raw = (d / "o.out").read_bytes()
    assert np.frombuffer(raw[:20], np.int32).tolist() == [2, 2, 2, 1, 1] and np.frombuffer(raw[20:40], np.int32).tolist() == [2, 2, 2, 1, 1]
    assert np.frombuffer(raw[40:], np.uint8).tolist() == [1, 1, 1, 1, 0]


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: an index past a plane, a list, a buffer pair or a dense array
    and signed overflow in the kernels' arithmetic end it"""
    exe, r = _build(tmp_path, "rivers_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    h = (tmp_path, exe)
    for name in ("single", "row", "column", "star", "star_t9", "star7", "comb", "empty", "serpentine_t8", "noise0_t1", "noise2_t8",
                 "noise3_t32"):
        for form in RV.FORMS:
            check_case(h, name, form)
