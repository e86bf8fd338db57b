"""The host side of the contours (gan_heightmaps_amd/contour.py): Levels' validation, the refusals that are made before
the device is touched, the launch sequence on a recording device inside one scratch, the max_segments refusal, the command lines'
parsing, the .npz / .svg / .geojson writers.  And the device code of csrc/contour.hip compiled for the CPU
(tests/contour_host/harness.cpp): the same source text the GPU runs -- the count, the scans, the links, both doublings, the lines
and the marks -- bit for bit against tests/contour_ref.py on the cases of the device tests, once more under the address and
undefined-behaviour sanitizers.  No device."""
import json
import os
import re
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from gan_heightmaps_amd import contour as CT
from tests import contour_ref as R
from tests.test_render_host import CSRC, ROOT, _compiler


# ---- validation -------------------------------------------------------------------------------------------------------------------
def test_levels_validation():
    lv = CT.Levels()
    assert (lv.interval, lv.base, lv.count, lv.index_every, lv.height_scale, lv.interval_q, lv.base_q) == (4.0, 0.0, None, 5, 64.0, 1024, 0)
    assert CT.Levels(np.float32(1.5), 1, np.int64(7), 2, 8) == CT.Levels(1.5, 1.0, 7, 2, 8.0) and hash(lv) == hash(CT.Levels())
    assert CT.Levels(interval=1 / 256).interval_q == 1 and CT.Levels(base=-2.0).base_q == -512 and CT.Levels(base=65536).base_q == 1 << 24
    assert CT.Levels(interval=1.5 / 256).interval_q == 2 and CT.Levels(interval=2.5 / 256).interval_q == 2          # half to even
    assert lv.height(3) == 12.0 and CT.Levels(2.0, -1.0).height(-2) == -5.0
    assert [lv.is_index(j) for j in (-5, -1, 0, 4, 5)] == [True, False, True, False, True]
    with pytest.raises(Exception):
        lv.interval = 3                                                    # frozen
    for kw in (dict(interval=0), dict(interval=-1), dict(interval=0.001), dict(interval=65537), dict(interval=None), dict(interval=True),
               dict(interval=float("nan")), dict(base=70000), dict(base=-70000), dict(base="1"), dict(base=float("inf")),
               dict(count=0), dict(count=-1), dict(count=1.5), dict(count=True), dict(count=(1 << 28) + 1), dict(index_every=0),
               dict(index_every=2.0), dict(index_every=None), dict(height_scale=0), dict(height_scale=65537), dict(height_scale=None)):
        with pytest.raises(ValueError):
            CT.Levels(**kw)
    assert CT.KEEP == ('zq',)


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    h = R.heights(8, 9, 1)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            CT.contours(ops, bad)
    x = h.copy()
    x[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        CT.contours(ops, x)
    for v in (-0.01, 1.5):
        x = h.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            CT.contours(ops, x)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        CT.contours(ops, huge)
    with pytest.raises(ValueError, match="Levels"):
        CT.contours(ops, h, dict(interval=2))
    for bad in (3, (1,), (1.5, 2), None):
        with pytest.raises(ValueError, match="origin"):
            CT.contours(ops, h, origin=bad)
    for bad in (-1, 1.5, None, 1 << 31):
        with pytest.raises(ValueError, match="max_segments"):
            CT.contours(ops, h, max_segments=bad)
    with pytest.raises(ValueError, match="keep"):
        CT.contours(ops, h, keep=('edge',))
    tex = np.zeros((8, 9, 3), np.uint8)
    for bad in ((1, 2), (1.5, 0, 0), None):
        with pytest.raises(ValueError, match="colour"):
            CT.paint(ops, tex, h, colour=bad)
    with pytest.raises(ValueError, match="opacity"):
        CT.paint(ops, tex, h, opacity=2)
    with pytest.raises(ValueError, match="opacity"):
        CT.paint(ops, tex, h, index_opacity=-0.5)
    with pytest.raises(ValueError, match="Levels"):
        CT.paint(ops, tex, h, levels=4.0)
    with pytest.raises(ValueError, match="zq"):
        CT.paint(ops, tex, hand_made())
    with pytest.raises(ValueError, match="non-finite"):
        CT.marks(ops, x * np.nan)


class Counting:
    """tests.fake_device.FakeDevice that counts what is live"""

    def __new__(cls):
        from tests.fake_device import FakeDevice

        class Dev(FakeDevice):
            def __init__(self):
                super().__init__()
                self.live, self.sizes = 0, []

            def alloc(self, nbytes):
                self.live += 1
                self.sizes.append(int(nbytes))
                return super().alloc(nbytes)

            def free(self, ptr):
                self.live -= 1

        return Dev()


def recording_ops(segments, lines, vertices):
    from tests.fake_device import RecordingOps

    class Ops(RecordingOps):
        def contour_cells_bytes(self, H, W):
            return 1000 + H * W

        def contour_workspace(self, H, W, S):
            return 5000 + 28 * S

        def contour_count(self, *args):
            self.calls.append(("contour_count", args, {}))
            return segments

        def contour_trace(self, *args):
            self.calls.append(("contour_trace", args, {}))
            return lines, vertices, 3

    return Ops(Counting())


def test_contours_sends_its_launches_inside_one_scratch():
    h = R.heights(20, 33, 1)
    ops = recording_ops(40, 3, 45)
    got = CT.contours(ops, h[None], CT.Levels(2.0, -1.0, 7, 2, 32.0), origin=(100, -10), keep='zq')
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "contour_count", "contour_trace", "contour_extract"] and ops.dev.live == 0
    qu, co, tr, ex = (c[1] for c in ops.calls)
    assert qu[1:5] == (33, 20, 33, 32.0) and qu[6] == 33
    assert co[0] == qu[5] and co[1:7] == (33, 20, 33, -256, 512, 7)
    assert tr[:8] == co and tr[9] == 40
    assert ex[:9] == tr[:9] and ex[9:12] == (40, 3, 45) and len(ex) == 17 and len(set(ex[12:])) == 5
    # the plane, its quantisation, the cells, the workspace, then the five arrays
    assert ops.dev.sizes == [2640, 2640, 1660, 5000 + 28 * 40, 45 * 12, 45 * 8, 4 * 8, 16, 16]
    assert got.shape == (20, 33) and got.origin == (100, -10) and len(got) == 3 and got.rounds == 3 and got.zq.dtype == np.int32
    assert got.edge.shape == (45, 3) and got.t.shape == (45,) and got.offsets.shape == (4,) and got.points.shape == (45, 2)
    assert "3 lines" in repr(got)
    # no cells and no segments: the same sequence, on arrays of no length
    ops = recording_ops(0, 0, 0)
    got = CT.contours(ops, (h[:1] * 255).astype(np.uint8))
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "contour_count", "contour_trace", "contour_extract"] and ops.dev.live == 0
    assert ops.calls[1][1][4:7] == (0, 1024, -1) and len(got) == 0 and got.segments().shape == (0,) and got.lines() == []


def test_more_segments_than_max_segments_are_refused_before_the_workspace():
    ops = recording_ops(41, 3, 45)
    with pytest.raises(ValueError, match="41 contour segments"):
        CT.contours(ops, R.heights(20, 33, 1), max_segments=40)
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "contour_count"] and ops.dev.live == 0
    assert ops.dev.sizes == [2640, 2640, 1660]                             # the workspace was never asked for
    ops = recording_ops(40, 3, 45)
    CT.contours(ops, R.heights(20, 33, 1), max_segments=40)


def test_the_paint_goes_through_the_hydrologys_kernel_twice():
    from tests.fake_device import FakeDevice, RecordingOps
    sent = []

    class Paint(RecordingOps):
        def hydrology_paint(self, *args):
            self.calls.append(("hydrology_paint", args, {}))

    class Dev(FakeDevice):
        def h2d(self, ptr, arr):
            sent.append(np.array(arr))

    ops = Paint(Dev())
    h = R.heights(8, 9, 2)
    out = CT.paint(ops, np.zeros((8, 9, 3), np.uint8), h, CT.Levels(1.0, index_every=3), (1.0, 0.0, 0.0), 0.5, 0.75)
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "contour_marks", "hydrology_paint", "hydrology_paint"]
    mk = ops.calls[1][1]
    assert mk[1:8] == (9, 8, 9, 0, 256, -1, 3) and mk[9] == 9
    first, second = ops.calls[2][1], ops.calls[3][1]
    assert first[10] == 0.5 and second[10] == 0.75 and first[12:14] == (1, 0) and second[12:14] == (2, 0)
    assert out.shape == (8, 9, 3) and out.dtype == np.uint8
    # a Contours that kept its heights is painted from them
    del ops.calls[:], sent[:]
    c = hand_made(zq=np.arange(12, dtype=np.int32).reshape(3, 4))
    CT.paint(ops, np.zeros((3, 4), np.float32), c)
    assert [k[0] for k in ops.calls] == ["contour_marks", "hydrology_paint", "hydrology_paint"]
    assert np.array_equal(sent[0], c.zq) and ops.calls[0][1][4:8] == (512, 1024, 3, 2)
    with pytest.raises(ValueError, match="height_scale"):
        CT.paint(ops, np.zeros((3, 4), np.float32), c, CT.Levels(height_scale=3.0))
    with pytest.raises(ValueError, match="differ in size"):
        CT.paint(ops, np.zeros((4, 3), np.float32), c)


# ---- the methods and the writers on a hand-made Contours ---------------------------------------------------------------------------
def hand_made(zq=None):
    """three lines in a 3 x 4 plane at (10, -20): an open one of three vertices, a loop of four, an open one of two"""
    edge = np.array([[0, 0, 1], [0, 0, 0], [0, 1, 1],
                     [1, 1, 0], [1, 2, 1], [2, 1, 0], [1, 1, 1],
                     [0, 2, 0], [0, 3, 1]], np.int32)
    t = np.array([0.25, 0.5, 0.75, 0.125, 0.375, 0.625, 0.875, 1 / 3, 0.1], np.float64)
    return CT.Contours(edge, t, np.array([0, 3, 7, 9], np.int64), np.array([0, 2, 1], np.int32), np.array([0, 1, 0], np.uint8),
                       CT.Levels(4.0, 2.0, 3, 2), (10, -20), (3, 4), 2, zq)


def test_contours_methods():
    c = hand_made()
    assert len(c) == 3 and c.shape == (3, 4) and c.origin == (10, -20)
    assert c.points.tolist()[:3] == [[10.25, -20.0], [10.0, -19.5], [10.75, -19.0]]
    assert c.line(1).tolist() == [[11.0, -18.875], [11.375, -18.0], [12.0, -18.375], [11.875, -19.0]]
    assert [c.height(i) for i in range(3)] == [2.0, 10.0, 6.0] and [c.is_index(i) for i in range(3)] == [True, True, False]
    assert c.lines() == [0, 1, 2] and c.lines(level=2) == [1] and c.lines(index_only=True) == [0, 1] and c.lines(5) == []
    for bad in (3, -1, 1.0, None):
        with pytest.raises(ValueError, match="line"):
            c.line(bad)
    s = c.segments()
    assert s.dtype == CT.SEGMENT and len(s) == 2 + 4 + 1 and s["level"].tolist() == [0, 0, 1, 2, 2, 2, 2]
    assert s["edge_p"][0].tolist() == [10, -20, 0] and s["edge_q"][0].tolist() == [10, -19, 1] and s["t_p"][0] == 0.5
    loop = s[s["level"] == 2]
    assert sorted(map(tuple, loop["edge_p"].tolist())) == sorted(map(tuple, loop["edge_q"].tolist()))          # it closes
    assert (11, -19, 1) in map(tuple, loop["edge_q"].tolist())
    # the segments of the cells inside a rectangle: the cell (10, -20) alone holds the first line
    inside = c.segments(within=(10, -20, 2, 2))
    assert inside["level"].tolist() == [0, 0] and len(c.segments(within=(10, -20, 3, 4))) == 7
    assert len(c.segments(within=(11, -19, 2, 2))) == 4 and len(c.segments(within=(10, -20, 1, 4))) == 0


def path_points(d):
    nums = [float(v) for v in re.findall(r"-?\d+(?:\.\d+)?(?:e-?\d+)?", d)]
    return [[nums[i + 1], nums[i]] for i in range(0, len(nums), 2)]


def test_the_writers(tmp_path):
    c = hand_made()
    c.save(str(tmp_path / "c.npz"))
    z = np.load(str(tmp_path / "c.npz"))
    for k in ("edge", "t", "offsets", "level", "closed"):
        assert np.array_equal(z[k], getattr(c, k)) and z[k].dtype == getattr(c, k).dtype
    assert z["origin"].tolist() == [10, -20] and z["shape"].tolist() == [3, 4] and z["levels"].tolist() == [4.0, 2.0, 3.0, 2.0, 64.0]
    tex = np.random.RandomState(1).randint(0, 256, (3, 4, 3)).astype(np.uint8)
    c.save(str(tmp_path / "c.svg"), texture=tex)
    root = ET.parse(str(tmp_path / "c.svg")).getroot()
    ns = "{http://www.w3.org/2000/svg}"
    assert root.tag == ns + "svg" and root.get("viewBox") == "-20 10 3 2"
    paths = root.findall(ns + "path")
    assert len(paths) == 3
    for i, p in enumerate(paths):
        assert path_points(p.get("d")) == c.line(i).tolist()                                         # repr round-trips a double
        assert p.get("d").rstrip().endswith("Z") == bool(c.closed[i]) and int(p.get("data-level")) == c.level[i]
        assert p.get("class") == ("index" if c.is_index(i) else "line")
    assert float(paths[0].get("stroke-width")) > float(paths[2].get("stroke-width"))
    img = root.find(ns + "image")
    import base64
    import io
    from PIL import Image
    data = img.get("{http://www.w3.org/1999/xlink}href")
    assert data.startswith("data:image/png;base64,") and (img.get("width"), img.get("height")) == ("4", "3")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(base64.b64decode(data.split(",", 1)[1])))), tex)
    c.save(str(tmp_path / "plain.svg"))
    assert ET.parse(str(tmp_path / "plain.svg")).getroot().find(ns + "image") is None
    with pytest.raises(ValueError, match="texture"):
        c.save(str(tmp_path / "bad.svg"), texture=np.zeros((4, 3), np.uint8))
    c.save(str(tmp_path / "c.geojson"))
    g = json.load(open(str(tmp_path / "c.geojson")))
    assert g["type"] == "FeatureCollection" and len(g["features"]) == 3
    for i, f in enumerate(g["features"]):
        want = [[col, row] for row, col in c.line(i).tolist()]
        assert f["geometry"]["type"] == "LineString" and f["geometry"]["coordinates"] == want + (want[:1] if c.closed[i] else [])
        assert f["properties"] == dict(level=int(c.level[i]), height=c.height(i), index=c.is_index(i), closed=bool(c.closed[i]))
    with pytest.raises(ValueError, match="npz, .svg or .geojson"):
        c.save(str(tmp_path / "c.txt"))


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = CT.parse_args(["in.png", "out.svg"])
    assert (a.input, a.output, a.levels, a.texture, a.painted) == ("in.png", "out.svg", CT.Levels(), None, None)
    a = CT.parse_args(["i.npy", "o.geojson", "--interval", "2.5", "--base", "-3", "--count", "4", "--index-every", "2", "--height-scale",
                       "32", "--texture", "t.png", "--painted", "p.png", "--colour", "0.5,0.25,0", "--opacity", "0.75"])
    assert a.levels == CT.Levels(2.5, -3.0, 4, 2, 32.0)
    assert (a.texture, a.painted, a.colour, a.opacity) == ("t.png", "p.png", (0.5, 0.25, 0.0), 0.75)
    assert CT.parse_args(["i", "o.NPZ", "--texture", "t.png"]).texture == "t.png"
    for bad in (["i"], ["i", "o.txt"], ["i", "o.svg", "--interval", "0"], ["i", "o.svg", "--interval", "x"], ["i", "o.svg", "--base", "70000"],
                ["i", "o.svg", "--count", "0"], ["i", "o.svg", "--count", "1.5"], ["i", "o.svg", "--index-every", "0"],
                ["i", "o.svg", "--height-scale", "0"], ["i", "o.svg", "--painted", "p.png"],
                ["i", "o.svg", "--texture", "t", "--painted", "p", "--colour", "2,0,0"],
                ["i", "o.svg", "--texture", "t", "--painted", "p", "--opacity", "1.5"]):
        with pytest.raises(SystemExit):
            CT.parse_args(bad)


def test_the_worlds_command_line_takes_contours():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    a = WD.parse_args(base)
    assert a.contours is None
    a = WD.parse_args(base + ["--contours", "lines.svg", "--interval", "2", "--base", "-1", "--count", "3", "--index-every", "4"])
    assert a.contours == "lines.svg" and a.levels == CT.Levels(2.0, -1.0, 3, 4)
    assert WD.parse_args(base + ["--contours", "lines.geojson"]).levels == CT.Levels()
    for bad in (["--contours", "lines.txt"], ["--interval", "2"], ["--contours", "l.svg", "--interval", "0"], ["--count", "2"],
                ["--contours", "l.npz", "--index-every", "0"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "contour.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "contour.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           '-DCONTOUR_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "contour_host", "harness.cpp"),
                                                              "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("contour_host")
    exe, r = _build(d, "contour_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_trace(harness, zq, base_q, interval_q, count, index_every):
    """-> (dict of the five arrays, segments and rounds, marks); zq goes in with rows of W + 3 cells whose padding is 2^30 high, the
    marks lie in rows of W + 2 cells whose padding must come back untouched"""
    d, exe = harness
    H, W = zq.shape
    wide = np.full((H, W + 3), 1 << 30, np.int32)
    wide[:, :W] = zq
    (d / "in.bin").write_bytes(wide.tobytes())
    args = ["trace", H, W, W + 3, W + 2, base_q, interval_q, -1 if count is None else count, index_every, d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    S, L, V, rounds = (int(v) for v in np.frombuffer(raw[:32], np.int64))
    at = [32]

    def take(dtype, n):
        a = np.frombuffer(raw[at[0]:at[0] + n * np.dtype(dtype).itemsize], dtype)
        at[0] += a.nbytes
        return a

    got = dict(edge=take(np.int32, 3 * V).reshape(V, 3), t=take(np.float64, V), offsets=take(np.int64, L + 1), level=take(np.int32, L),
               closed=take(np.uint8, L), segments=S, rounds=rounds)
    planes = np.frombuffer(raw[at[0]:], np.uint8).reshape(H, (W + 2) * 4)
    assert (planes[:, W * 4:] == 0xAB).all(), "cells beyond a row's width were written"
    return got, np.ascontiguousarray(planes[:, :W * 4]).view(np.uint32).reshape(H, W)


def ranking_rounds(longest):
    """the rounds of pointer doubling over a longest line of this many segments, the one that changes nothing included"""
    return 0 if longest == 0 else max(longest - 2, 0).bit_length() + 1


def same_lines(got, want):
    for k in ("edge", "offsets", "level", "closed"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["t"].view(np.int64), want["t"].view(np.int64)), "t"
    assert got["segments"] == want["segments"]
    return True


def check_case(harness, name):
    c = R.case(name)
    want, want_marks = R.expected(name)
    got, got_marks = run_trace(harness, c["zq"], c["base_q"], c["interval_q"], c["count"], c["index_every"])
    assert same_lines(got, want), name
    assert got["rounds"] == ranking_rounds(want["longest"]), name
    assert np.array_equal(got_marks, want_marks), name
    return want


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_trace_and_the_marks_on_the_host_build(harness, name):
    want = check_case(harness, name)
    if name == "serpentine":
        assert want["segments"] == 4604 and want["closed"].tolist() == [1] and ranking_rounds(4604) >= 13
    if name in ("row", "column"):
        assert want["segments"] == 0 and len(want["level"]) == 0 and want["offsets"].tolist() == [0]


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: an index past a cell, segment or line array and signed
    overflow in the kernels' arithmetic end it"""
    exe, r = _build(tmp_path, "contour_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    h = (tmp_path, exe)
    for name in ("row", "column", "peak", "steep", "steep_diag", "tie", "saddle_a_above", "saddle_b_below", "noise37", "integers",
                 "serpentine_open", "clipped", "negative_base"):
        check_case(h, name)
    # the largest heights the quantisation gives against the lowest base, one level apart: the int64 arithmetic has room
    zq = np.zeros((5, 6), np.int32)
    zq[::2, ::2] = 1 << 24
    zq[1, 1] = -(1 << 24)
    for base_q, iq, count in ((-(1 << 24), 1 << 20, None), (1 << 24, 1 << 22, None), (0, 1, 3), ((1 << 24) - 2, 1, 5)):
        got, got_marks = run_trace(h, zq, base_q, iq, count, 5)
        assert same_lines(got, R.trace(zq, base_q, iq, count)) and np.array_equal(got_marks, R.marks(zq, base_q, iq, count, 5))
