"""The host side of the peaks (gan_heightmaps_amd/peaks.py): Prominence's validation, the refusals that are made before
the device is touched, the launch sequence on a recording device inside one scratch, the max_summits refusal, the Peaks' methods
and writers, Contours.save(peaks=...), both command lines.  And the device code of csrc/peaks.hip compiled for the CPU
(tests/peaks_host/harness.cpp): the same source text the GPU runs -- the ascent, the count, the scans, the Boruvka rounds in both
forms, the extraction -- and ghm_peaks_merge's body, bit for bit against tests/peaks_ref.py on the cases of the device tests, once
more under the address and undefined-behaviour sanitizers.  No device."""
import csv
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from gan_heightmaps_amd import contour as CT
from gan_heightmaps_amd import peaks as PK
from tests import peaks_ref as R
from tests.test_render_host import CSRC, ROOT, _compiler


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_prominence_validation():
    p = PK.Prominence()
    assert (p.min_prominence, p.top, p.height_scale, p.min_q) == (8.0, None, 64.0, 2048)
    assert PK.Prominence(np.float32(1.5), np.int64(3), 8) == PK.Prominence(1.5, 3, 8.0) and hash(p) == hash(PK.Prominence())
    assert PK.Prominence(0).min_q == 1 and PK.Prominence(0.001).min_q == 1 and PK.Prominence(1.5 / 256).min_q == 2
    with pytest.raises(Exception):
        p.top = 3                                                          # frozen
    for kw in (dict(min_prominence=-1), dict(min_prominence=65537), dict(min_prominence=None), dict(min_prominence=True),
               dict(min_prominence=float("nan")), dict(min_prominence="8"), dict(top=0), dict(top=-1), dict(top=1.5), dict(top=True),
               dict(top=1 << 31), dict(height_scale=0), dict(height_scale=65537), dict(height_scale=None)):
        with pytest.raises(ValueError):
            PK.Prominence(**kw)
    assert PK.KEEP == ('zq', 'label') and PK.FORMS == ('plain', 'list') and PK.DEFAULT_FORM in PK.FORMS


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    h = R.heights(8, 9, 1)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            PK.peaks(ops, bad)
    x = h.copy()
    x[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        PK.peaks(ops, x)
    for v in (-0.01, 1.5):
        x = h.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            PK.peaks(ops, x)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        PK.peaks(ops, huge)
    with pytest.raises(ValueError, match="Prominence"):
        PK.peaks(ops, h, 8.0)
    for bad in (3, (1,), (1.5, 2), None):
        with pytest.raises(ValueError, match="origin"):
            PK.peaks(ops, h, origin=bad)
    for bad in ("tiled", 0, True):
        with pytest.raises(ValueError, match="form"):
            PK.peaks(ops, h, form=bad)
    for bad in (-1, 1.5, None, 1 << 31):
        with pytest.raises(ValueError, match="max_summits"):
            PK.peaks(ops, h, max_summits=bad)
    with pytest.raises(ValueError, match="keep"):
        PK.peaks(ops, h, keep=('area',))
    tex = np.zeros((3, 7, 3), np.uint8)
    for bad in ((1, 2), (1.5, 0, 0), None):
        with pytest.raises(ValueError, match="colour"):
            PK.paint(ops, tex, hand_made(), colour=bad)
    for bad in (-1, 5, 1.0):
        with pytest.raises(ValueError, match="radius"):
            PK.paint(ops, tex, hand_made(), radius=bad)
    with pytest.raises(ValueError, match="Peaks"):
        PK.paint(ops, tex, h)


# ---- the launch sequence ------------------------------------------------------------------------------------------------------------
def recording_ops(summits, edges):
    from tests.fake_device import RecordingOps
    from tests.test_contour_host import Counting

    class Ops(RecordingOps):
        def hydrology_workspace(self, H, W):
            return 256 + 24 * H * W

        def peaks_workspace(self, H, W):
            return 1000 + 28 * H * W

        def peaks_list_bytes(self, E):
            return 500 + 20 * E

        def hydrology_accumulate(self, *args):
            self.calls.append(("hydrology_accumulate", args, {}))
            return 4

        def peaks_count(self, *args):
            self.calls.append(("peaks_count", args, {}))
            return summits, edges

        def peaks_tree(self, *args):
            self.calls.append(("peaks_tree", args, {}))
            return 3

        def peaks_merge(self, summit, summit_zq, tree, saddle_zq, min_zq):
            self.calls.append(("peaks_merge", (len(summit), len(tree), min_zq), {}))
            P = len(summit)
            return np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.arange(P, dtype=np.int32) * 4096

    return Ops(Counting())


SEQUENCE = ["viewshed_quantise", "peaks_ascent", "hydrology_accumulate", "peaks_count", "peaks_tree", "peaks_extract", "peaks_merge"]


def test_peaks_sends_its_launches_inside_one_scratch():
    h = R.heights(20, 33, 1)
    ops = recording_ops(5, 40)
    got = PK.peaks(ops, h[None], PK.Prominence(2.0, None, 32.0), origin=(100, -10), form='list', keep=('zq', 'label'))
    assert [c[0] for c in ops.calls] == SEQUENCE and ops.dev.live == 0
    qu, asc, acc, co, tr, ex, me = (c[1] for c in ops.calls)
    assert qu[1:5] == (33, 20, 33, 32.0) and qu[6] == 33
    d_z = qu[5]
    assert asc[:4] == (d_z, 33, 20, 33) and asc[5] == 33
    d_dir = asc[4]
    assert acc[:4] == (d_dir, 33, 20, 33) and acc[5] == 33 and acc[7] == 33
    d_area, d_label = acc[4], acc[6]
    assert co[:6] == (d_z, 33, d_label, 33, 20, 33)
    d_w = co[6]
    assert tr[:7] == (d_z, 33, d_label, 33, 20, 33, 1) and tr[8] == 33 and tr[9] == d_w and tr[11:13] == (5, 40)
    d_m, d_l = tr[7], tr[10]
    assert ex[:9] == (d_label, 33, d_area, 33, d_m, 33, 20, 33, d_w) and ex[9] == 5 and len(set(ex[10:])) == 3
    assert me == (5, 4, 0)
    # the plane, its quantisation, direction, area, label, the hydrology's workspace, the peaks', mask, list, then the three arrays
    n = 20 * 33
    assert ops.dev.sizes == [4 * n, 4 * n, n, 4 * n, 4 * n, 256 + 24 * n, 1000 + 28 * n, 4 * n, 500 + 20 * 40, 20, 20, 48]
    assert d_l is not None and len({d_z, d_dir, d_area, d_label, d_w, d_m, d_l}) == 7
    assert got.shape == (20, 33) and got.origin == (100, -10) and got.summits == 5 and got.rounds == 3 and got.form == 'list'
    assert len(got) == 4 and got.prominence.tolist() == [64.0, 48.0, 32.0, 16.0]          # the fake's prominence 0 is dropped
    assert got.zq.dtype == np.int32 and got.label.shape == (20, 33) and "4 peaks of 5 summits" in repr(got)
    # the plain form allocates no list
    ops = recording_ops(1, 0)
    got = PK.peaks(ops, (h * 255).astype(np.uint8), form='plain')
    assert [c[0] for c in ops.calls] == SEQUENCE and ops.dev.live == 0 and len(ops.dev.sizes) == 11
    assert ops.calls[4][1][6] == 0 and ops.calls[4][1][10] is None and len(got) == 0 and got.zq is None and got.label is None
    assert got.passes() == [] and got.observers() == []


def test_more_summits_than_max_summits_are_refused_before_the_tree():
    ops = recording_ops(41, 300)
    with pytest.raises(ValueError, match="41 summits"):
        PK.peaks(ops, R.heights(20, 33, 1), max_summits=40)
    assert [c[0] for c in ops.calls] == SEQUENCE[:4] and ops.dev.live == 0
    assert len(ops.dev.sizes) == 7                                         # no mask, no list, no array of the extraction
    ops = recording_ops(40, 300)
    PK.peaks(ops, R.heights(20, 33, 1), max_summits=40)


def test_the_paint_goes_through_the_hydrologys_kernel():
    from tests.fake_device import FakeDevice, RecordingOps
    sent = []

    class Dev(FakeDevice):
        def h2d(self, ptr, arr):
            sent.append(np.array(arr))

    ops = RecordingOps(Dev())
    p = hand_made()
    out = PK.paint(ops, np.zeros((3, 7, 3), np.uint8), p, (1.0, 0.0, 0.0), 1)
    assert [c[0] for c in ops.calls] == ["hydrology_paint"] and out.shape == (3, 7, 3) and out.dtype == np.uint8
    marks = [a for a in sent if a.dtype == np.uint32][0]
    assert np.argwhere(marks.reshape(3, 7) == 1).tolist() == [[1, 1], [1, 5]] and marks.sum() == 2
    del sent[:], ops.calls[:]
    PK.paint(ops, np.zeros((3, 7), np.float32), p, cols=True)
    marks = [a for a in sent if a.dtype == np.uint32][0]
    assert np.argwhere(marks.reshape(3, 7) == 1).tolist() == [[1, 3]]
    with pytest.raises(ValueError, match="differ in size"):
        PK.paint(ops, np.zeros((4, 3), np.float32), p)


# ---- the methods and the writers on a hand-made Peaks --------------------------------------------------------------------------------
def hand_made(origin=(10, -20)):
    """the two peaks of the case two_peaks at ``origin``, every summit reported"""
    e = R.expected("two_peaks")
    z = e["zq"].ravel() * 256
    return PK.report(e["summit"], z[e["summit"]], e["col"], z[np.maximum(e["col"], 0)], e["parent"], e["prominence_q"] * 256,
                     e["summit_area"], PK.Prominence(1.0), origin, e["zq"].shape, rounds=1, form='plain')


def test_peaks_methods():
    p = hand_made()
    assert len(p) == 2 and p.shape == (3, 7) and p.origin == (10, -20) and p.summits == 2
    assert p.cell.tolist() == [[11, -19], [11, -15]] and p.cell.dtype == np.int64
    assert p.height.tolist() == [9.0, 7.0] and p.prominence.tolist() == [9.0, 4.0]
    assert np.isnan(p.col_height[0]) and p.col_height[1] == 3.0 and p.col.tolist() == [[-1, -1], [11, -17]]
    assert p.parent.tolist() == [-1, 0] and p.parent.dtype == np.int32 and p.on_edge.tolist() == [0, 0] and p.area.dtype == np.uint32
    assert int(p.area.sum()) == 21
    assert p.observers() == [(11, -19), (11, -15)] and p.observers(2) == [(11, -19, 2.0), (11, -15, 2.0)]
    assert p.passes() == [(11, -17)] and p.lineage(1) == [1, 0] and p.lineage(0) == [0]
    for bad in (2, -1, 1.0, None):
        with pytest.raises(ValueError, match="peak"):
            p.lineage(bad)
    # a col at (-1, -1) of another origin is a col all the same
    q = hand_made(origin=(-2, -4))
    assert q.col.tolist() == [[-1, -1], [-1, -1]] and q.passes() == [(-1, -1)]
    # the filter and the order: min_prominence, top, the parents re-numbered
    e = R.expected("row")
    z = e["zq"].ravel()
    args = (e["summit"], z[e["summit"]], e["col"], z[np.maximum(e["col"], 0)], e["parent"], e["prominence_q"], e["summit_area"])
    got = PK.report(*args, PK.Prominence(0), (0, 0), (1, 9))
    assert got.cell[:, 1].tolist() == [5, 7, 2, 0] and got.parent.tolist() == [-1, 0, 0, 0] and got.on_edge.tolist() == [1, 1, 1, 1]
    got = PK.report(*args, PK.Prominence(3 / 256, 2), (0, 0), (1, 9))
    assert got.cell[:, 1].tolist() == [5, 7] and got.summits == 4
    assert PK.report(*args, PK.Prominence(3.5 / 256), (0, 0), (1, 9)).cell[:, 1].tolist() == [5, 7]


def test_the_writers(tmp_path):
    p = hand_made()
    p.save(str(tmp_path / "p.npz"))
    z = np.load(str(tmp_path / "p.npz"))
    for k in ("cell", "height", "prominence", "col", "parent", "area", "on_edge"):
        assert np.array_equal(z[k], getattr(p, k)) and z[k].dtype == getattr(p, k).dtype
    assert z["origin"].tolist() == [10, -20] and z["shape"].tolist() == [3, 7] and z["rule"].tolist() == [1.0, -1.0, 64.0]
    p.save(str(tmp_path / "p.csv"))
    rows = list(csv.DictReader(open(str(tmp_path / "p.csv"))))
    assert [(int(r["row"]), int(r["col"]), float(r["height"]), float(r["prominence"]), int(r["parent"])) for r in rows] == [
        (11, -19, 9.0, 9.0, -1), (11, -15, 7.0, 4.0, 0)]
    assert (rows[1]["col_row"], rows[1]["col_col"], float(rows[1]["col_height"])) == ("11", "-17", 3.0) and rows[0]["col_height"] == "nan"
    p.save(str(tmp_path / "p.geojson"))
    g = json.load(open(str(tmp_path / "p.geojson")))
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 2
    f0, f1 = g["features"]
    assert f0["geometry"] == {"type": "Point", "coordinates": [-19, 11]} and f1["geometry"]["coordinates"] == [-15, 11]
    assert f1["properties"] == dict(height=7.0, prominence=4.0, col=[-17, 11], col_height=3.0, parent=0, area=int(p.area[1]),
                                    on_edge=False)
    assert f0["properties"]["col"] is None and f0["properties"]["col_height"] is None and f0["properties"]["parent"] == -1
    with pytest.raises(ValueError, match="npz, .csv or .geojson"):
        p.save(str(tmp_path / "p.svg"))


def sheet(origin=(10, -20)):
    """a Contours of the 3 x 7 plane of hand_made: one open line"""
    edge = np.array([[0, 0, 1], [0, 0, 0], [0, 1, 1]], np.int32)
    return CT.Contours(edge, np.array([0.25, 0.5, 0.75]), np.array([0, 3], np.int64), np.array([1], np.int32), np.array([0], np.uint8),
                       CT.Levels(4.0), origin, (3, 7), 2)


def test_contours_save_takes_the_peaks(tmp_path):
    c, p = sheet(), hand_made()
    # without peaks both files are byte for byte what the untouched _svg and _geojson give
    c.save(str(tmp_path / "a.svg"))
    assert open(str(tmp_path / "a.svg")).read() == c._svg(None)
    c.save(str(tmp_path / "a.geojson"), peaks=None)
    assert open(str(tmp_path / "a.geojson")).read() == json.dumps(c._geojson())
    c.save(str(tmp_path / "b.svg"), peaks=p)
    text = open(str(tmp_path / "b.svg")).read()
    assert text.startswith(c._svg(None)[:-len("</svg>\n")]) and text.endswith("</svg>\n")
    root = ET.parse(str(tmp_path / "b.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    assert len(root.findall(ns + "path")) == 1
    dots, texts = root.findall(ns + "circle"), root.findall(ns + "text")
    assert [(d.get("class"), d.get("cx"), d.get("cy")) for d in dots] == [("peak", "-19", "11"), ("peak", "-15", "11")]
    assert [t.text for t in texts] == ["9", "7"]
    c.save(str(tmp_path / "b.geojson"), peaks=p)
    g = json.load(open(str(tmp_path / "b.geojson")))
    assert [f["geometry"]["type"] for f in g["features"]] == ["LineString", "Point", "Point"]
    assert g["features"][:1] == c._geojson()["features"] and g["features"][1:] == p.features()
    for bad in (hand_made(origin=(0, 0)), "peaks", PK.report(*[np.zeros(0, np.int32)] * 7, PK.Prominence(), (10, -20), (4, 7))):
        with pytest.raises(ValueError, match="Peaks of the contours' plane"):
            c.save(str(tmp_path / "c.svg"), peaks=bad)
    with pytest.raises(ValueError, match="npz"):
        c.save(str(tmp_path / "c.npz"), peaks=p)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = PK.parse_args(["in.png", "out.geojson"])
    assert (a.input, a.output, a.prominence, a.texture, a.painted, a.form, a.cols) == ("in.png", "out.geojson", PK.Prominence(), None,
                                                                                      None, None, False)
    a = PK.parse_args(["i.npy", "o.csv", "--min-prominence", "2.5", "--top", "4", "--height-scale", "32", "--texture", "t.png",
                       "--painted", "p.png", "--colour", "0.5,0.25,0", "--radius", "3", "--cols", "--plain"])
    assert a.prominence == PK.Prominence(2.5, 4, 32.0) and (a.texture, a.painted, a.colour, a.radius, a.cols, a.form) == (
        "t.png", "p.png", (0.5, 0.25, 0.0), 3, True, "plain")
    assert PK.parse_args(["i", "o.NPZ", "--list"]).form == "list"
    for bad in (["i"], ["i", "o.svg"], ["i", "o.csv", "--min-prominence", "-1"], ["i", "o.csv", "--min-prominence", "x"],
                ["i", "o.csv", "--top", "0"], ["i", "o.csv", "--top", "1.5"], ["i", "o.csv", "--height-scale", "0"],
                ["i", "o.csv", "--painted", "p.png"], ["i", "o.csv", "--texture", "t.png"], ["i", "o.csv", "--plain", "--list"],
                ["i", "o.csv", "--texture", "t", "--painted", "p", "--colour", "2,0,0"],
                ["i", "o.csv", "--texture", "t", "--painted", "p", "--radius", "9"]):
        with pytest.raises(SystemExit):
            PK.parse_args(bad)


def test_the_worlds_command_line_takes_peaks():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    assert WD.parse_args(base).peaks is None
    a = WD.parse_args(base + ["--peaks", "tops.geojson", "--min-prominence", "2", "--top", "10"])
    assert a.peaks == "tops.geojson" and a.prominence == PK.Prominence(2.0, 10)
    assert WD.parse_args(base + ["--peaks", "tops.csv"]).prominence == PK.Prominence()
    a = WD.parse_args(base + ["--peaks", "tops.npz", "--contours", "sheet.svg"])
    assert (a.peaks, a.contours) == ("tops.npz", "sheet.svg")
    for bad in (["--peaks", "tops.svg"], ["--min-prominence", "2"], ["--top", "3"], ["--peaks", "t.csv", "--min-prominence", "-1"],
                ["--peaks", "t.csv", "--top", "0"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "peaks.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "peaks.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
           '-DPEAKS_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "peaks_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("peaks_host")
    exe, r = _build(d, "peaks_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_case(harness, zq, form):
    """-> dict of everything the harness gives; zq goes in with rows of W + 3 cells whose padding is 2^30 high, the planes come back in
    rows of W + 2 cells whose padding must be untouched"""
    d, exe = harness
    H, W = zq.shape
    wide = np.full((H, W + 3), 1 << 30, np.int32)
    wide[:, :W] = zq
    (d / "in.bin").write_bytes(wide.tobytes())
    args = ["run", H, W, W + 3, W + 2, PK.FORMS.index(form), d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    P, T, rounds, E, jumps = (int(v) for v in np.frombuffer(raw[:40], np.int64))
    at = [40]

    def take(dtype, n):
        a = np.frombuffer(raw[at[0]:at[0] + n * np.dtype(dtype).itemsize], dtype)
        at[0] += a.nbytes
        return a

    def plane(dtype):
        a = take(np.uint8, H * (W + 2) * np.dtype(dtype).itemsize).reshape(H, -1)
        assert (a[:, W * np.dtype(dtype).itemsize:] == 0xAB).all(), "cells beyond a row's width were written"
        return np.ascontiguousarray(a[:, :W * np.dtype(dtype).itemsize]).view(dtype).reshape(H, W)

    got = dict(ascent=plane(np.int8), label=plane(np.int32), area=plane(np.uint32), mask=plane(np.uint32), summit=take(np.int32, P),
               summit_area=take(np.uint32, P), tree=take(np.int32, 3 * T).reshape(T, 3), col=take(np.int32, P),
               parent=take(np.int32, P), prominence_q=take(np.int32, P), rounds=rounds, edges=E, jumps=jumps)
    assert at[0] == len(raw)
    return got


def check_case(harness, name, form):
    want = R.expected(name)
    got = run_case(harness, want["zq"], form)
    for k in ("ascent", "label", "area", "summit", "summit_area", "tree", "col", "parent", "prominence_q"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, form, k)
    assert got["rounds"] == want["rounds"] and got["edges"] == len(R.edges(want["zq"], want["label"])), (name, form)
    # the mask holds the tree's rows and nothing else
    H, W = want["zq"].shape
    bits = sum(bin(int(v)).count("1") for v in got["mask"].ravel())
    assert bits == len(want["tree"]) and set(np.flatnonzero(got["mask"].ravel()).tolist()) == set(want["tree"][:, 0].tolist())
    return got


@pytest.mark.parametrize("form", PK.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_on_the_host_build(harness, name, form):
    got = check_case(harness, name, form)
    if name == "ruler":
        assert got["rounds"] == 6
    if name == "staircase":
        assert got["rounds"] == 1 and got["jumps"] >= 2


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: an index past a plane, a list or a summit array and signed
    overflow in the kernels' arithmetic end it"""
    exe, r = _build(tmp_path, "peaks_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    h = (tmp_path, exe)
    for name in ("single", "row", "column", "flat", "triple", "lambda", "ruler", "staircase", "noise37", "extremes"):
        for form in PK.FORMS:
            check_case(h, name, form)
